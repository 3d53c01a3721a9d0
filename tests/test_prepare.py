"""Preparing correlator dumps without a GPU: ``rfi.host.PrepareHost`` against known answers
and a triple loop of float32 scalars, argument errors, slot wiring and every launch argument
on the fake backend, the sequence prepare -> fused flagger -> accumulate -> finalise, and the
argument checks of ``ksp_prepare``, which come before any device call."""

import ctypes

import numpy as np
import pytest

from katsdpsigproc_amd import accel
from katsdpsigproc_amd.rfi import device, host, ingest
from tests.fakes import FakeContext

LOST = -(2**31)
FULL = device.BackgroundFlags.FULL
f32 = np.float32


@pytest.fixture
def context():
    return FakeContext()


@pytest.fixture
def queue(context):
    return context.create_command_queue()


def dump(pairs):
    """int32 (1, len(pairs), 2) from a list of (re, im)."""
    return np.array([pairs], np.int32)


def arange32(n):
    return np.arange(n, dtype=np.int32)


def same_bits(want, got):
    assert want.dtype == got.dtype and want.shape == got.shape
    np.testing.assert_array_equal(np.ascontiguousarray(want).view(np.uint8),
                                  np.ascontiguousarray(got).view(np.uint8))  # fmt: skip


# ------------------------------------------------------------------------ known answers
def test_rounding_to_nearest_even():
    values = [2**24 + 1, 2**24 + 3, 2**31 - 1, -(2**31) + 1]
    vis_in = dump([(v, -v) for v in values])
    vis, flags, weights = host.PrepareHost()(vis_in, arange32(4))
    assert weights is None
    assert (vis.dtype, flags.dtype) == (np.complex64, np.uint8)
    assert vis.shape == flags.shape == (1, 4)
    want = [2.0**24, 2.0**24 + 4, 2.0**31, -(2.0**31)]  # ties to even; the last two round up
    assert vis.real[0].tolist() == want
    assert vis.imag[0].tolist() == [-w for w in want]
    assert not flags.any()
    # one more rounding by the multiplication, and the scale is taken as float32
    third = f32(1.0 / 3.0)
    vis, _, _ = host.PrepareHost(scale=1.0 / 3.0)(vis_in, arange32(4))
    assert vis.real[0, 1] == f32(f32(2.0**24 + 4) * third)
    assert vis.real[0, 1] != (2**24 + 3) / 3.0


def test_sentinel_in_re_and_in_im():
    vis_in = dump([(LOST, 5), (7, LOST), (LOST, LOST), (-(2**31) + 1, 2**31 - 1), (0, 0)])
    vis, flags, _ = host.PrepareHost(scale=0.5, lost_flag=0x10)(vis_in, arange32(5))
    assert flags[0].tolist() == [0x10, 0, 0x10, 0, 0]
    assert vis[0].tolist() == [0j, complex(3.5, -(2.0**30)), 0j, complex(-(2.0**30), 2.0**30), 0j]
    # a lost sample is +0.0 in both parts, not -0.0 and not the scaled imaginary part
    assert vis.view(np.uint32)[0, [0, 1, 4, 5]].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("index", [-1, 3, LOST, 2**31 - 1])
def test_invalid_source(index):
    vis_in = dump([(1, 2), (3, 4), (5, 6)])
    source = np.array([2, index, 0, 2], np.int32)
    vis, flags, _ = host.PrepareHost()(vis_in, source)
    assert vis[0].tolist() == [5 + 6j, 0j, 1 + 2j, 5 + 6j]  # a gather: repeats are allowed
    assert flags[0].tolist() == [0, 8, 0, 0]


def test_channel_flags_are_ored_with_lost_flag():
    vis_in = np.zeros((4, 2, 2), np.int32)
    vis_in[:, 1, 0] = LOST
    channel_flags = np.array([0, 0x01, 0x0C, 0x04], np.uint8)  # 0x0C and 0x04 overlap 0x0C
    _, flags, _ = host.PrepareHost(lost_flag=0x0C)(vis_in, arange32(2), channel_flags)
    assert flags.tolist() == [[0, 0x0C], [0x01, 0x0D], [0x0C, 0x0C], [0x04, 0x0C]]
    _, flags, _ = host.PrepareHost(lost_flag=0x0C)(vis_in, arange32(2))
    assert flags.tolist() == [[0, 0x0C]] * 4


# ----------------------------------------------------------------------- the triple loop
def triple_loop(vis_in, source, channel_flags, auto_source, scale, lost_flag, weight_scale):
    """The issue's arithmetic, sample by sample, in np.float32 scalars."""
    channels, in_baselines, _ = vis_in.shape
    baselines = len(source)
    scale, weight_scale = f32(scale), f32(weight_scale)
    vis = np.zeros((channels, baselines), np.complex64)
    flags = np.zeros((channels, baselines), np.uint8)
    weights = np.zeros((channels, baselines), f32) if auto_source is not None else None

    def power(c, k):
        if 0 <= k < in_baselines and vis_in[c, k, 0] != LOST:
            return f32(f32(vis_in[c, k, 0]) * scale)
        return f32(0)

    with np.errstate(all="ignore"):
        for c in range(channels):
            for j in range(baselines):
                s = int(source[j])
                lost = not 0 <= s < in_baselines or vis_in[c, s, 0] == LOST
                if not lost:
                    vis[c, j] = complex(f32(f32(vis_in[c, s, 0]) * scale),
                                        f32(f32(vis_in[c, s, 1]) * scale))  # fmt: skip
                f = int(channel_flags[c]) if channel_flags is not None else 0
                flags[c, j] = f | (lost_flag if lost else 0)
                if auto_source is not None:
                    pa = power(c, int(auto_source[j, 0]))
                    pb = power(c, int(auto_source[j, 1]))
                    d = f32(pa * pb)
                    if pa > 0 and pb > 0 and d > 0:
                        weights[c, j] = f32(weight_scale / d)
    return vis, flags, weights


def loop_case(seed=5):
    """5 x 9 from 13 input baselines: sentinels, invalid indices, every kind of power."""
    rs = np.random.RandomState(seed)
    channels, in_baselines, baselines = 5, 13, 9
    vis_in = rs.randint(-(2**31) + 1, 2**31, (channels, in_baselines, 2), np.int64).astype(np.int32)
    vis_in[rs.random_sample((channels, in_baselines)) < 0.15, 0] = LOST
    vis_in[rs.random_sample((channels, in_baselines)) < 0.15, 1] = LOST
    vis_in[:, :4, 0] = rs.randint(1, 2**20, (channels, 4))  # autocorrelations: positive
    vis_in[1, 0, 0] = 0
    vis_in[2, 1, 0] = -17
    vis_in[3, 2, 0] = LOST
    source = np.array([12, 4, 4, -1, 0, 13, 7, 5, 2**31 - 1], np.int32)
    auto_source = np.array([[0, 1], [1, 1], [2, 3], [3, 0], [0, 0], [-1, 2], [2, 13], [1, 3],
                            [0, 2]], np.int32)  # fmt: skip
    channel_flags = np.array([0, 1, 0, 0x88, 0], np.uint8)
    return vis_in, source, channel_flags, auto_source


@pytest.mark.parametrize("scale, weight_scale", [(1.0, 1.0), (1.0 / 3.0, 7.0), (2.0**-8, 2.0**20)])
@pytest.mark.parametrize("use_channel_flags", [False, True])
@pytest.mark.parametrize("use_weights", [False, True])
def test_host_against_triple_loop(use_weights, use_channel_flags, scale, weight_scale):
    vis_in, source, channel_flags, auto_source = loop_case()
    channel_flags = channel_flags if use_channel_flags else None
    auto_source = auto_source if use_weights else None
    got = host.PrepareHost(scale, 0x28, weight_scale)(vis_in, source, channel_flags, auto_source)
    want = triple_loop(vis_in, source, channel_flags, auto_source, scale, 0x28, weight_scale)
    same_bits(want[0], got[0])
    same_bits(want[1], got[1])
    if use_weights:
        same_bits(want[2], got[2])
        assert got[2].flags.c_contiguous
        assert (got[2] == 0).any() and (got[2] > 0).any() and np.isfinite(got[2]).all()
    else:
        assert got[2] is None
    assert (got[1] & 0x28).any() and not (got[1] & 0x28).all()


# ------------------------------------------------------------------------------ weights
def weight_of(re_a, re_b, scale=1.0, weight_scale=1.0, auto=(0, 1), lost_sample=False):
    """The weight of one output baseline whose autocorrelations have real parts `re_a`, `re_b`."""
    vis_in = dump([(re_a, 3), (re_b, -3), (LOST if lost_sample else 11, 1)])
    vis, flags, weights = host.PrepareHost(scale, 8, weight_scale)(
        vis_in, np.array([2], np.int32), None, np.array([auto], np.int32))
    assert weights.dtype == f32 and weights.shape == (1, 1)
    assert flags[0, 0] == (8 if lost_sample else 0)
    return weights[0, 0]


def is_plus_zero(x):
    return x == 0 and not np.signbit(x)


def test_weight_known_answers():
    assert weight_of(4, 8) == f32(1.0 / 32.0)
    assert weight_of(4, 8, scale=0.5, weight_scale=3.0) == f32(0.375)
    assert weight_of(3, 1, weight_scale=1.0) == f32(1.0) / f32(3.0)  # correctly rounded
    assert weight_of(5, 7, auto=(0, 0)) == f32(1.0) / f32(25.0)  # an autocorrelation itself
    # a lost sample keeps the weight of its baseline
    assert weight_of(4, 8, lost_sample=True) == f32(1.0 / 32.0)


def test_weight_zero_autocorrelation():
    assert is_plus_zero(weight_of(0, 8)) and is_plus_zero(weight_of(8, 0))


def test_weight_negative_autocorrelation():
    assert is_plus_zero(weight_of(-4, 8)) and is_plus_zero(weight_of(8, -4))
    assert is_plus_zero(weight_of(-4, -8))  # the product is positive, the powers are not


def test_weight_sentinel_autocorrelation():
    assert is_plus_zero(weight_of(LOST, 8)) and is_plus_zero(weight_of(8, LOST))


@pytest.mark.parametrize("index", [-1, 3, LOST, 2**31 - 1])
def test_weight_invalid_auto_source(index):
    assert is_plus_zero(weight_of(4, 8, auto=(index, 1)))
    assert is_plus_zero(weight_of(4, 8, auto=(0, index)))


def test_weight_overflow_of_the_product():
    # powers near 2^31 * 2^40 = 2^71 each: d is inf, 1 / inf is +0.0
    assert is_plus_zero(weight_of(2**31 - 1, 2**31 - 1, scale=2.0**40))
    assert weight_of(2**31 - 1, 1, scale=2.0**40) > 0  # (2^111 is still a float32)


def test_weight_underflow_of_the_product():
    # powers of 2^-80 each: d = 2^-160 is 0 in float32, and the weight is 0, not inf
    assert is_plus_zero(weight_of(1, 1, scale=2.0**-80))
    # a denormal product is a product: the quotient overflows as IEEE says, no NaN anywhere
    assert weight_of(1, 1, scale=2.0**-70) == np.inf


# ------------------------------------------------------------------------------- errors
def test_host_errors():
    for bad in (0.0, -1.0, np.nan, np.inf, 1e39, 1e-46):  # (1e39 is inf, 1e-46 is 0 as float32)
        with pytest.raises(ValueError, match="scale"):
            host.PrepareHost(scale=bad)
        with pytest.raises(ValueError, match="weight_scale"):
            host.PrepareHost(weight_scale=bad)
    assert host.PrepareHost(scale=0.1).scale == f32(0.1)
    assert type(host.PrepareHost(scale=2).scale) is f32
    for bad in (0, 256, -1):
        with pytest.raises(ValueError, match="lost_flag"):
            host.PrepareHost(lost_flag=bad)
    for bad in (1.0, True, "8"):
        with pytest.raises(TypeError, match="lost_flag"):
            host.PrepareHost(lost_flag=bad)
    prepare = host.PrepareHost()
    vis_in = np.zeros((4, 6, 2), np.int32)
    source = arange32(5)
    channel_flags = np.zeros(4, np.uint8)
    auto_source = np.zeros((5, 2), np.int32)
    prepare(vis_in, source, channel_flags, auto_source)
    for name, bad in [
        ("vis_in", vis_in.astype(np.int64)), ("vis_in", vis_in.astype(np.float32)),
        ("vis_in", vis_in[..., 0]), ("vis_in", np.zeros((4, 6, 3), np.int32)),
        ("vis_in", np.zeros((0, 6, 2), np.int32)), ("vis_in", np.zeros((4, 0, 2), np.int32)),
        ("source", source.astype(np.int64)), ("source", source[:, np.newaxis]),
        ("source", source[:0]),
        ("channel_flags", channel_flags.astype(bool)), ("channel_flags", channel_flags[:3]),
        ("channel_flags", np.zeros((4, 5), np.uint8)),
        ("auto_source", auto_source.astype(np.uint32)), ("auto_source", auto_source[:4]),
        ("auto_source", auto_source.T), ("auto_source", auto_source[:, 0]),
    ]:  # fmt: skip
        args = {"vis_in": vis_in, "source": source, "channel_flags": channel_flags,
                "auto_source": auto_source}  # fmt: skip
        args[name] = bad
        with pytest.raises(ValueError, match=name):
            prepare(**args)


def test_template_and_operation_errors(context, queue):
    for kwargs in ({"scale": 0.0}, {"scale": np.nan}, {"weight_scale": -1.0}, {"weight_scale": np.inf},
                   {"lost_flag": 0}, {"lost_flag": 256}):  # fmt: skip
        with pytest.raises(ValueError):
            ingest.PrepareTemplate(context, **kwargs)
    with pytest.raises(TypeError):
        ingest.PrepareTemplate(context, lost_flag=1.5)
    with pytest.raises(ValueError):
        ingest.PrepareTemplate(context, tuning={"wgs": 256})
    assert ingest.PrepareTemplate(context, tuning={}).tuning == {}
    assert ingest.PrepareTemplate.autotune(context) == {}
    assert ingest.PrepareTemplate.host_class is host.PrepareHost
    assert ingest.PrepareTemplate.KERNEL == "ksp_prepare"
    template = ingest.PrepareTemplate(context)
    for args in [(0, 4), (4, 0), (-4, 4), (4, 4, 0), (4, 4, -1)]:
        with pytest.raises(ValueError):
            template.instantiate(queue, *args)
    assert template.instantiate(queue, 4, 5).in_baselines == 5
    assert template.instantiate(queue, 4, 5, 3).in_baselines == 3
    assert isinstance(template.instantiate(queue, 4, 5, in_baselines=9), ingest.Prepare)


def test_host_from_device_errors(context, queue):
    vis_in = np.zeros((4, 6, 2), np.int32)
    source = arange32(5)
    channel_flags = np.zeros(4, np.uint8)
    auto_source = np.zeros((5, 2), np.int32)
    plain = ingest.PrepareHostFromDevice(ingest.PrepareTemplate(context), queue)
    with pytest.raises(TypeError, match="channel_flags"):
        plain(vis_in, source, channel_flags)
    with pytest.raises(TypeError, match="auto_source"):
        plain(vis_in, source, auto_source=auto_source)
    both = ingest.PrepareHostFromDevice(
        ingest.PrepareTemplate(context, channel_flags=True, weights=True), queue)
    with pytest.raises(TypeError, match="channel_flags"):
        both(vis_in, source, auto_source=auto_source)
    with pytest.raises(TypeError, match="auto_source"):
        both(vis_in, source, channel_flags)
    vis, flags, weights = plain(vis_in, source)
    assert vis.shape == flags.shape == (4, 5) and weights is None
    assert [out.shape for out in both(vis_in, source, channel_flags, auto_source)] == [(4, 5)] * 3
    assert [name for name, _ in queue.launches] == ["ksp_prepare"] * 2
    assert [int(a) for a in queue.launches[0][1][7:10]] == [4, 6, 5]


# ------------------------------------------------------------------------------- wiring
@pytest.mark.parametrize("use_channel_flags", [False, True])
@pytest.mark.parametrize("use_weights", [False, True])
def test_wiring(use_weights, use_channel_flags, context, queue):
    template = ingest.PrepareTemplate(context, scale=0.1, lost_flag=0x40,
                                      channel_flags=use_channel_flags, weights=use_weights,
                                      weight_scale=3.0)  # fmt: skip
    fn = template.instantiate(queue, 300, 200, 250)
    shapes = {"vis_in": (300, 250, 2), "source": (200,), "vis": (300, 200),
              "input_flags": (300, 200)}  # fmt: skip
    if use_channel_flags:
        shapes["channel_flags"] = (300,)
    if use_weights:
        shapes.update({"auto_source": (200, 2), "weights": (300, 200)})
    dtypes = {"vis_in": np.int32, "source": np.int32, "channel_flags": np.uint8,
              "auto_source": np.int32, "vis": np.complex64, "input_flags": np.uint8,
              "weights": np.float32}  # fmt: skip
    assert set(fn.slots) == set(shapes)
    for name, shape in shapes.items():
        assert fn.slots[name].shape == shape and fn.slots[name].dtype == dtypes[name]
    # the pairs are never padded apart
    assert fn.slots["vis_in"].dimensions[2].exact
    assert not use_weights or fn.slots["auto_source"].dimensions[1].exact
    # a dimension object of its own for everything that can be padded
    dims = [d for slot in fn.slots.values() for d in slot.dimensions]
    assert len({id(d) for d in dims}) == len(dims)
    accel.Dimension(200, min_padded_size=500).link(fn.slots["input_flags"].dimensions[1])
    accel.Dimension(250, min_padded_size=260).link(fn.slots["vis_in"].dimensions[1])
    fn()
    assert [name for name, _ in queue.launches] == ["ksp_prepare"]
    args = queue.launches[0][1]
    assert len(args) == 17
    assert args[0] is fn.buffer("vis_in").buffer and args[1] is fn.buffer("source").buffer
    assert args[2] is (fn.buffer("auto_source").buffer if use_weights else None)
    assert args[3] is (fn.buffer("channel_flags").buffer if use_channel_flags else None)
    assert args[4] is fn.buffer("vis").buffer and args[5] is fn.buffer("input_flags").buffer
    assert args[6] is (fn.buffer("weights").buffer if use_weights else None)
    assert [int(a) for a in args[7:10]] == [300, 250, 200]
    assert all(isinstance(a, np.int32) for a in args[7:14]) and isinstance(args[16], np.int32)

    def padded(name):
        return fn.buffer(name).padded_shape

    assert [int(a) for a in args[10:14]] == [
        padded("vis_in")[1], padded("vis")[1], padded("input_flags")[1],
        padded("weights")[1] if use_weights else 0]  # fmt: skip
    assert padded("vis_in") == (300, 260, 2)
    assert padded("vis")[1] == 208 and padded("input_flags")[1] == 512  # whole 128-byte rows
    if use_weights:
        assert padded("weights")[1] == 224 and padded("auto_source")[1] == 2
    assert isinstance(args[14], np.float32) and args[14] == f32(0.1)
    assert isinstance(args[15], np.float32) and args[15] == f32(3.0)
    assert int(args[16]) == 0x40
    assert fn.parameters() == {
        "scale": float(f32(0.1)), "lost_flag": 0x40, "channel_flags": use_channel_flags,
        "weights": use_weights, "weight_scale": 3.0, "in_baselines": 250, "channels": 300,
        "baselines": 200}  # fmt: skip


def test_in_front_of_the_chain(context, queue):
    """prepare -> fused flagger (FULL) -> accumulate (weights, FULL) -> finalise: `vis`,
    `input_flags` and `weights` are each one buffer with one padded size."""
    channels, baselines, in_baselines = 4096, 200, 260
    prepare = ingest.PrepareTemplate(context, weights=True, channel_flags=True).instantiate(
        queue, channels, baselines, in_baselines)  # fmt: skip
    flagger = device.FlaggerDeviceTemplate(
        device.BackgroundMedianFilterDeviceTemplate(context, 13, use_flags=FULL),
        device.NoiseEstMADTDeviceTemplate(context, channels),
        device.ThresholdSumDeviceTemplate(context),
        tuning={"vis_pad": 0},
    ).instantiate(queue, channels, baselines, threshold_args={"n_sigma": 11.0})
    assert isinstance(flagger, device.FusedFlaggerDevice)
    accumulate = device.AccumulateTemplate(context, input_flags=FULL).instantiate(
        queue, channels, baselines)  # fmt: skip
    finalise = device.FinaliseTemplate(context, channel_factor=8).instantiate(
        queue, channels, baselines)  # fmt: skip
    # more row padding than any of them asks for, asked of another member of each compound
    accel.Dimension(baselines, min_padded_size=300).link(flagger.slots["vis"].dimensions[1])
    accel.Dimension(baselines, min_padded_size=400).link(accumulate.slots["input_flags"].dimensions[1])
    accel.Dimension(baselines, min_padded_size=500).link(prepare.slots["weights"].dimensions[1])
    seq = accel.OperationSequence(
        queue,
        [("prepare", prepare), ("flagger", flagger), ("accumulate", accumulate),
         ("finalise", finalise)],
        compounds={
            "vis": ["prepare:vis", "flagger:vis", "accumulate:vis"],
            "input_flags": ["prepare:input_flags", "flagger:input_flags",
                            "accumulate:input_flags"],
            "weights": ["prepare:weights", "accumulate:weights"],
            "flags": ["flagger:flags", "accumulate:flags"],
            "acc_vis": ["accumulate:acc_vis", "finalise:acc_vis"],
            "acc_weights": ["accumulate:acc_weights", "finalise:acc_weights"],
            "acc_flags": ["accumulate:acc_flags", "finalise:acc_flags"],
        })  # fmt: skip
    for name in ("prepare:vis", "flagger:vis", "accumulate:weights", "prepare:input_flags"):
        assert name not in seq.slots
    assert {"prepare:vis_in", "prepare:source", "prepare:auto_source",
            "prepare:channel_flags"} <= set(seq.slots)  # fmt: skip
    for name in device.FusedFlaggerDevice._OPTIONAL:
        del seq.slots["flagger:" + name]
    seq()
    assert [name for name, _ in queue.launches] == [
        "ksp_prepare", "ksp_flagger_fused", "ksp_average_accumulate", "ksp_average_finalise"]  # fmt: skip
    prep_args, flag_args, add_args, _ = (launch[1] for launch in queue.launches)
    for name in ("vis", "input_flags"):
        assert prepare.buffer(name) is flagger.buffer(name) is accumulate.buffer(name)
        assert prepare.buffer(name) is seq.buffer(name)
    assert prepare.buffer("weights") is accumulate.buffer("weights") is seq.buffer("weights")
    assert prep_args[4] is flag_args[0] is add_args[0] is seq.buffer("vis").buffer
    assert prep_args[5] is flag_args[1] is add_args[3] is seq.buffer("input_flags").buffer
    assert prep_args[6] is add_args[2] is seq.buffer("weights").buffer
    assert int(add_args[4]) == FULL.value
    vis_stride = seq.buffer("vis").padded_shape[1]
    mask_stride = seq.buffer("input_flags").padded_shape[1]
    weights_stride = seq.buffer("weights").padded_shape[1]
    # 300, 400 and 500 rounded up to whole 128-byte rows
    assert (vis_stride, mask_stride, weights_stride) == (304, 512, 512)
    assert int(prep_args[11]) == int(flag_args[7]) == int(add_args[10]) == vis_stride
    assert int(prep_args[12]) == int(flag_args[8]) == int(add_args[13]) == mask_stride
    assert int(prep_args[13]) == int(add_args[12]) == weights_stride
    assert int(prep_args[10]) == in_baselines


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

    def call(vis_in=p, source=p, auto_source=p, channel_flags=p, vis=p, input_flags=p, weights=p,
             channels=4, in_baselines=8, baselines=8, vis_in_stride=8, vis_stride=8,
             input_flags_stride=8, weights_stride=8, scale=1.0, weight_scale=1.0, lost_flag=8):  # fmt: skip
        rc = lib.ksp_prepare(
            0, None, vis_in, source, auto_source, channel_flags, vis, input_flags, weights,
            channels, in_baselines, baselines, vis_in_stride, vis_stride, input_flags_stride,
            weights_stride, scale, weight_scale, lost_flag)  # fmt: skip
        assert rc != 0
        return _lib.last_error()

    assert "invalid argument: vis_in is NULL" in call(vis_in=None)
    assert "invalid argument: source is NULL" in call(source=None)
    assert "invalid argument: vis is NULL" in call(vis=None)
    assert "invalid argument: input_flags is NULL" in call(input_flags=None)
    assert "auto_source and weights must both" in call(auto_source=None)
    assert "auto_source and weights must both" in call(weights=None)
    assert "channels must be" in call(channels=0)
    assert "in_baselines must be" in call(in_baselines=0)
    assert "invalid argument: baselines must be" in call(baselines=0)
    assert "invalid argument: vis_in_stride is smaller than in_baselines" in call(vis_in_stride=7)
    for name in ("vis", "input_flags", "weights"):
        assert f"invalid argument: {name}_stride is smaller than baselines" in call(
            **{name + "_stride": 7})  # fmt: skip
    # the order of the checks: everything wrong at once, then only every stride
    strides = dict(vis_in_stride=-1, vis_stride=-1, input_flags_stride=-1, weights_stride=-1)
    assert "invalid argument: vis_in is NULL" in call(
        vis_in=None, source=None, auto_source=None, channel_flags=None, vis=None,
        input_flags=None, weights=None, channels=0, in_baselines=0, baselines=0, **strides)  # fmt: skip
    assert "invalid argument: vis_in_stride is smaller than in_baselines" in call(**strides)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert "invalid argument: scale must be finite" in call(scale=bad)
        assert "weight_scale must be finite" in call(weight_scale=bad)
    for bad in (0, 256, -8):
        assert "lost_flag must be 1..255" in call(lost_flag=bad)
    # what belongs to the weights is not looked at without them
    message = call(auto_source=None, weights=None, weights_stride=0, weight_scale=0.0,
                   lost_flag=0)  # fmt: skip
    assert "lost_flag" in message
    # 2^31 - 1 rows of 2^31 - 1 baselines: more workgroups than a grid has
    assert "too large for one launch" in call(
        channels=2**31 - 1, in_baselines=1, baselines=2**31 - 1, vis_in_stride=1,
        vis_stride=2**31 - 1, input_flags_stride=2**31 - 1, weights_stride=2**31 - 1)  # fmt: skip
