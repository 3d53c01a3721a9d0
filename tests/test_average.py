"""Flag-aware averaging without a GPU: the NumPy class against known answers and a triple
loop of float32 scalars, argument errors, slot wiring on the fake backend, the sequence
behind the fused flagger, and the argument checks of ``ksp_average_accumulate`` and
``ksp_average_finalise``, which come before any device call."""

import ctypes

import numpy as np
import pytest

from katsdpsigproc_amd import accel, rfi
from katsdpsigproc_amd.rfi import device, host
from tests.fakes import FakeContext

NONE, CHANNEL, FULL = (device.BackgroundFlags.NONE, device.BackgroundFlags.CHANNEL,
                       device.BackgroundFlags.FULL)  # fmt: skip


@pytest.fixture
def context():
    return FakeContext()


@pytest.fixture
def queue(context):
    return context.create_command_queue()


def test_background_flags_is_one_class():
    assert device.BackgroundFlags is host.BackgroundFlags is rfi.BackgroundFlags
    assert [m.value for m in device.BackgroundFlags] == [0, 1, 2]
    assert not NONE and CHANNEL and FULL


@pytest.mark.parametrize("dumps, want", [
    ([(2 + 4j, 0, 1), (4 + 8j, 0, 3)], (3.5 + 7j, 4, 0)),
    ([(1 + 1j, 0, 2), (100 + 100j, 4, 2)], (1 + 1j, 2, 0)),  # the flagged sample is absorbed
    ([(100 + 100j, 4, 2), (1 + 1j, 0, 2)], (1 + 1j, 2, 0)),  # ... in either order
    ([(3 + 4j, 2, 1.5), (1 + 0j, 8, 0.5)], (2.5 + 3j, 2, 10)),
    ([(5 + 5j, 0, 0)], (0j, 0, 0)),
    ([(3 + 4j, 2, 1.5)], (3 + 4j, 1.5, 2)),
])  # fmt: skip
def test_known_answers(dumps, want):
    averager = host.AveragerHost(1, 1)
    for vis, flags, weight in dumps:
        averager.add(np.array([[vis]], np.complex64), np.array([[flags]], np.uint8),
                     np.array([[weight]], np.float32))  # fmt: skip
    vis, weights, flags = averager.finalise()
    assert (vis.dtype, weights.dtype, flags.dtype) == (np.complex64, np.float32, np.uint8)
    assert vis.shape == weights.shape == flags.shape == (1, 1)
    assert (vis[0, 0], weights[0, 0], flags[0, 0]) == want


def make_dumps(rs, n_dumps, channels, baselines):
    """[(vis, flags, weights)]: about half the samples flagged, some zero weights."""
    dumps = []
    for _ in range(n_dumps):
        vis = (rs.standard_normal((channels, baselines))
               + 1j * rs.standard_normal((channels, baselines))).astype(np.complex64)  # fmt: skip
        flags = np.where(rs.random_sample((channels, baselines)) < 0.5,
                         rs.randint(1, 256, (channels, baselines)), 0).astype(np.uint8)  # fmt: skip
        weights = rs.uniform(0.5, 2.0, (channels, baselines)).astype(np.float32)
        weights[rs.random_sample((channels, baselines)) < 0.1] = 0
        dumps.append((vis, flags, weights))
    return dumps


def triple_loop(dumps, masks, channels, baselines, channel_factor):
    """The issue's arithmetic, sample by sample, in np.float32 scalars."""
    f32 = np.float32
    acc_re = np.zeros((channels, baselines), f32)
    acc_im = np.zeros((channels, baselines), f32)
    acc_w = np.zeros((channels, baselines), f32)
    acc_f = np.zeros((channels, baselines), np.uint8)
    for (vis, flags, weights), mask in zip(dumps, masks):
        for c in range(channels):
            for b in range(baselines):
                f = int(flags[c, b])
                if mask is not None:
                    f |= int(mask[c] if mask.ndim == 1 else mask[c, b])
                w = f32(1) if weights is None else f32(weights[c, b])
                we = f32(w * f32(2.0**-64)) if f else w
                acc_re[c, b] = f32(acc_re[c, b] + f32(we * f32(vis[c, b].real)))
                acc_im[c, b] = f32(acc_im[c, b] + f32(we * f32(vis[c, b].imag)))
                acc_w[c, b] = f32(acc_w[c, b] + we)
                acc_f[c, b] |= f
    rows = channels // channel_factor
    out_vis = np.zeros((rows, baselines), np.complex64)
    out_w = np.zeros((rows, baselines), f32)
    out_f = np.zeros((rows, baselines), np.uint8)
    for r in range(rows):
        for b in range(baselines):
            re, im, w, fl = f32(0), f32(0), f32(0), 0
            for k in range(channel_factor):
                c = r * channel_factor + k
                re, im, w = f32(re + acc_re[c, b]), f32(im + acc_im[c, b]), f32(w + acc_w[c, b])
                fl |= int(acc_f[c, b])
            allbad = w < f32(2.0**-32)
            if allbad:
                w, re, im = f32(w * f32(2.0**64)), f32(re * f32(2.0**64)), f32(im * f32(2.0**64))
            if w > 0:
                out_vis[r, b] = complex(f32(re / w), f32(im / w))
            out_w[r, b] = w
            out_f[r, b] = fl if allbad else 0
    return out_vis, out_w, out_f


def same_bits(want, got):
    assert want.dtype == got.dtype and want.shape == got.shape
    np.testing.assert_array_equal(want.view(np.uint8), got.view(np.uint8))


@pytest.mark.parametrize("mode", [NONE, CHANNEL, FULL])
@pytest.mark.parametrize("channel_factor", [1, 3, 12])
def test_host_against_triple_loop(channel_factor, mode):
    channels, baselines = 12, 7
    rs = np.random.RandomState(channel_factor * 3 + mode.value)
    dumps = make_dumps(rs, 5, channels, baselines)
    dumps[2] = dumps[2][:2] + (None,)  # one dump without weights
    for _, flags, _ in dumps:
        flags[:, 0] = 0  # a column that only the mask can flag
        flags[:, 1] |= 0x10  # a column flagged in every dump
    if mode == NONE:
        masks = [None] * 5
    else:
        shape = (channels,) if mode == CHANNEL else (channels, baselines)
        masks = [np.where(rs.random_sample(shape) < 0.3, 0x40, 0).astype(np.uint8) for _ in dumps]
    averager = host.AveragerHost(channels, baselines, channel_factor, mode)
    for (vis, flags, weights), mask in zip(dumps, masks):
        kwargs = {} if mask is None else {"input_flags": mask}
        averager.add(vis, flags, weights, **kwargs)
    vis, weights, flags = averager.finalise()
    want = triple_loop(dumps, masks, channels, baselines, channel_factor)
    for w, g in zip(want, (vis, weights, flags)):
        same_bits(w, g)
    assert flags[:, 1].all() and np.all(weights[:, 1] > 0)
    assert flags.any() and not flags.all()
    # state is zero after finalise: a second finalise reports "no data" everywhere
    assert not averager.acc_vis.any() and not averager.acc_weights.any()
    assert not averager.acc_flags.any()
    assert averager.acc_vis.dtype == np.complex64 and averager.acc_weights.dtype == np.float32
    assert averager.acc_flags.dtype == np.uint8
    for out in averager.finalise():
        assert out.shape == (channels // channel_factor, baselines) and not out.any()


def test_mode_by_value():
    assert host.AveragerHost(4, 4, input_flags=1).input_flags is CHANNEL
    with pytest.raises(ValueError):
        host.AveragerHost(4, 4, input_flags=3)


def test_host_errors():
    for args in [(0, 4), (4, 0), (-1, 4), (4, 4, 0), (4, 4, -1), (4, 4, 3), (4, 4, 8)]:
        with pytest.raises(ValueError):
            host.AveragerHost(*args)
    vis = np.zeros((4, 3), np.complex64)
    flags = np.zeros((4, 3), np.uint8)
    with pytest.raises(TypeError):
        host.AveragerHost(4, 3).add(vis, flags, input_flags=np.zeros(4, np.uint8))
    for mode in (CHANNEL, FULL):
        with pytest.raises(TypeError):
            host.AveragerHost(4, 3, input_flags=mode).add(vis, flags)
    with pytest.raises(ValueError):
        host.AveragerHost(4, 3, input_flags=CHANNEL).add(vis, flags, input_flags=flags)
    with pytest.raises(ValueError):
        host.AveragerHost(4, 3, input_flags=FULL).add(vis, flags, input_flags=flags[:, 0])
    with pytest.raises(ValueError):
        host.AveragerHost(4, 3).add(vis[:2], flags[:2])


def test_template_errors(context, queue):
    accumulate = device.AccumulateTemplate(context)
    finalise = device.FinaliseTemplate(context, channel_factor=4)
    for channels, baselines in [(0, 4), (4, 0), (-4, 4)]:
        with pytest.raises(ValueError):
            accumulate.instantiate(queue, channels, baselines)
        with pytest.raises(ValueError):
            finalise.instantiate(queue, channels, baselines)
    for channels in (2, 6, 9):
        with pytest.raises(ValueError):
            finalise.instantiate(queue, channels, 4)
    for channel_factor in (0, -2):
        with pytest.raises(ValueError):
            device.FinaliseTemplate(context, channel_factor=channel_factor)
    with pytest.raises(ValueError):
        device.AccumulateTemplate(context, input_flags=5)
    for cls in (device.AccumulateTemplate, device.FinaliseTemplate):
        with pytest.raises(ValueError):
            cls(context, tuning={"wgs": 256})
        assert cls(context, tuning={}).tuning == {}
        assert cls.autotune(context) == {}
        assert cls.host_class is host.AveragerHost


def test_host_from_device_errors(context, queue):
    vis = np.zeros((4, 3), np.complex64)
    flags = np.zeros((4, 3), np.uint8)
    finalise = device.FinaliseTemplate(context)
    plain = device.AveragerHostFromDevice(device.AccumulateTemplate(context), finalise, queue, 4, 3)
    with pytest.raises(TypeError):
        plain.add(vis, flags, input_flags=np.zeros(4, np.uint8))
    masked = device.AveragerHostFromDevice(
        device.AccumulateTemplate(context, input_flags=CHANNEL), finalise, queue, 4, 3)
    with pytest.raises(TypeError):
        masked.add(vis, flags)
    with pytest.raises(ValueError):
        device.AveragerHostFromDevice(device.AccumulateTemplate(context),
                                      device.FinaliseTemplate(context, 3), queue, 4, 3)  # fmt: skip
    # one set of accumulators, shared by the two operations; kernels in call order
    plain.add(vis, flags)
    plain.finalise()
    assert [name for name, _ in queue.launches] == ["ksp_average_accumulate",
                                                    "ksp_average_finalise"]  # fmt: skip
    add_args, fin_args = queue.launches[0][1], queue.launches[1][1]
    assert add_args[5] is fin_args[0] and add_args[6] is fin_args[1] and add_args[7] is fin_args[2]


@pytest.mark.parametrize("mode", [NONE, CHANNEL, FULL])
@pytest.mark.parametrize("use_weights", [True, False])
def test_accumulate_wiring(use_weights, mode, context, queue):
    template = device.AccumulateTemplate(context, use_weights=use_weights, input_flags=mode)
    fn = template.instantiate(queue, 300, 200)
    names = {"vis", "flags", "acc_vis", "acc_weights", "acc_flags"}
    names |= {"weights"} if use_weights else set()
    names |= {"input_flags"} if mode else set()
    assert set(fn.slots) == names
    dtypes = {"vis": np.complex64, "flags": np.uint8, "weights": np.float32,
              "input_flags": np.uint8, "acc_vis": np.complex64, "acc_weights": np.float32,
              "acc_flags": np.uint8}  # fmt: skip
    for name in names:
        shape = (300,) if (name == "input_flags" and mode == CHANNEL) else (300, 200)
        assert fn.slots[name].shape == shape and fn.slots[name].dtype == dtypes[name]
    # a dimension object of its own per slot: padding one does not pad another
    dims = [fn.slots[name].dimensions[1] for name in names if len(fn.slots[name].shape) == 2]
    assert len({id(d) for d in dims}) == len(dims)
    accel.Dimension(200, min_padded_size=500).link(fn.slots["acc_weights"].dimensions[1])
    fn()
    assert [name for name, _ in queue.launches] == ["ksp_average_accumulate"]
    args = queue.launches[0][1]
    assert len(args) == 17
    assert args[0] is fn.buffer("vis").buffer and args[1] is fn.buffer("flags").buffer
    assert args[2] is (fn.buffer("weights").buffer if use_weights else None)
    assert args[3] is (fn.buffer("input_flags").buffer if mode else None)
    assert int(args[4]) == mode.value
    assert args[5] is fn.buffer("acc_vis").buffer
    assert args[6] is fn.buffer("acc_weights").buffer
    assert args[7] is fn.buffer("acc_flags").buffer
    assert [int(a) for a in args[8:10]] == [300, 200]

    def stride(name):
        return fn.buffer(name).padded_shape[1]

    assert [int(a) for a in args[10:]] == [
        stride("vis"), stride("flags"), stride("weights") if use_weights else 0,
        stride("input_flags") if mode == FULL else 0, stride("acc_vis"), stride("acc_weights"),
        stride("acc_flags")]  # fmt: skip
    # rows of whole 128 bytes, except where more was asked for
    assert stride("vis") == stride("acc_vis") == 208
    assert stride("flags") == stride("acc_flags") == 256
    assert stride("acc_weights") == 512
    assert fn.parameters() == {"use_weights": use_weights, "input_flags": mode.name,
                               "channels": 300, "baselines": 200}  # fmt: skip


@pytest.mark.parametrize("clear", [True, False])
def test_finalise_wiring(clear, context, queue):
    fn = device.FinaliseTemplate(context, channel_factor=4, clear=clear).instantiate(queue, 300, 200)
    names = ["acc_vis", "acc_weights", "acc_flags", "vis", "weights", "flags"]
    assert list(fn.slots) == names
    for name, dtype in zip(names, [np.complex64, np.float32, np.uint8] * 2):
        assert fn.slots[name].shape == ((300, 200) if name.startswith("acc_") else (75, 200))
        assert fn.slots[name].dtype == dtype
    accel.Dimension(200, min_padded_size=300).link(fn.slots["flags"].dimensions[1])
    fn()
    assert [name for name, _ in queue.launches] == ["ksp_average_finalise"]
    args = queue.launches[0][1]
    assert len(args) == 16
    for arg, name in zip(args, names):
        assert arg is fn.buffer(name).buffer
    assert [int(a) for a in args[6:10]] == [300, 200, 4, int(clear)]
    assert [int(a) for a in args[10:]] == [fn.buffer(name).padded_shape[1] for name in names]
    assert [int(a) for a in args[10:]] == [208, 224, 256, 208, 224, 384]
    assert fn.parameters() == {"channel_factor": 4, "clear": clear, "channels": 300,
                               "baselines": 200}  # fmt: skip


def test_behind_the_fused_flagger(context, queue):
    channels, baselines = 4096, 200
    flagger = device.FlaggerDeviceTemplate(
        device.BackgroundMedianFilterDeviceTemplate(context, 13, use_flags=CHANNEL),
        device.NoiseEstMADTDeviceTemplate(context, channels),
        device.ThresholdSumDeviceTemplate(context),
        tuning={"vis_pad": 0},
    ).instantiate(queue, channels, baselines, threshold_args={"n_sigma": 11.0})
    assert isinstance(flagger, device.FusedFlaggerDevice)
    accumulate = device.AccumulateTemplate(context, input_flags=CHANNEL).instantiate(
        queue, channels, baselines)  # fmt: skip
    finalise = device.FinaliseTemplate(context, channel_factor=8).instantiate(
        queue, channels, baselines)  # fmt: skip
    # more row padding than any of them asks for, as a caller's own requirement would
    accel.Dimension(baselines, min_padded_size=300).link(accumulate.slots["flags"].dimensions[1])
    accel.Dimension(baselines, min_padded_size=300).link(flagger.slots["vis"].dimensions[1])
    seq = accel.OperationSequence(
        queue, [("flagger", flagger), ("accumulate", accumulate), ("finalise", finalise)],
        compounds={
            "vis": ["flagger:vis", "accumulate:vis"],
            "flags": ["flagger:flags", "accumulate:flags"],
            "input_flags": ["flagger:input_flags", "accumulate:input_flags"],
            "acc_vis": ["accumulate:acc_vis", "finalise:acc_vis"],
            "acc_weights": ["accumulate:acc_weights", "finalise:acc_weights"],
            "acc_flags": ["accumulate:acc_flags", "finalise:acc_flags"],
        })  # fmt: skip
    for name in ("flagger:vis", "accumulate:vis", "flagger:flags", "accumulate:flags"):
        assert name not in seq.slots
    assert seq.slots["vis"].shape == seq.slots["flags"].shape == (channels, baselines)
    # a sequence allocates every slot it shows, the flagger's optional temporaries included
    # (which then get computed); a caller who does not want them takes them off the list
    for name in device.FusedFlaggerDevice._OPTIONAL:
        del seq.slots["flagger:" + name]
    seq()
    assert [name for name, _ in queue.launches] == [
        "ksp_flagger_fused", "ksp_average_accumulate", "ksp_average_finalise"]  # fmt: skip
    flag_args, add_args, fin_args = (launch[1] for launch in queue.launches)
    assert flag_args[3] is None  # no deviations asked of the flagger
    # one buffer and one padded size for both users of vis and of flags
    assert flagger.buffer("vis") is accumulate.buffer("vis") is seq.buffer("vis")
    assert flagger.buffer("flags") is accumulate.buffer("flags") is seq.buffer("flags")
    assert flag_args[0] is add_args[0] and flag_args[2] is add_args[1]
    assert flag_args[1] is add_args[3] is seq.buffer("input_flags").buffer
    vis_stride = seq.buffer("vis").padded_shape[1]
    flags_stride = seq.buffer("flags").padded_shape[1]
    assert vis_stride == 304 and flags_stride == 384  # 300 rounded up to 128-byte rows
    assert int(flag_args[7]) == int(add_args[10]) == vis_stride
    assert int(flag_args[9]) == int(add_args[11]) == flags_stride
    # the accumulators go from the accumulation to the finishing pass
    assert add_args[5] is fin_args[0] and add_args[6] is fin_args[1] and add_args[7] is fin_args[2]
    assert seq.buffer("finalise:vis").shape == (channels // 8, baselines)


@pytest.fixture(scope="module")
def lib():
    import os

    from katsdpsigproc_amd import _lib, build_native

    if not os.path.exists(_lib.LIB_PATH):
        build_native.build()
    return _lib.load()


def test_accumulate_argument_validation_without_gpu(lib):
    from katsdpsigproc_amd import _lib

    p = ctypes.c_void_p(64)  # never dereferenced: every call below fails its checks first

    def call(vis=p, flags=p, weights=p, input_flags=None, mode=0, acc_vis=p, acc_weights=p,
             acc_flags=p, channels=4, baselines=8, vis_stride=8, flags_stride=8, weights_stride=8,
             input_flags_stride=8, acc_vis_stride=8, acc_weights_stride=8, acc_flags_stride=8):  # fmt: skip
        rc = lib.ksp_average_accumulate(
            0, None, vis, flags, weights, input_flags, mode, acc_vis, acc_weights, acc_flags,
            channels, baselines, vis_stride, flags_stride, weights_stride, input_flags_stride,
            acc_vis_stride, acc_weights_stride, acc_flags_stride)  # fmt: skip
        assert rc != 0
        return _lib.last_error()

    small = "_stride is smaller than baselines"
    assert "invalid argument: vis is NULL" in call(vis=None) and "acc_vis" not in _lib.last_error()
    assert "invalid argument: flags is NULL" in call(flags=None)
    assert "invalid argument: acc_vis is NULL" in call(acc_vis=None)
    assert "invalid argument: acc_weights is NULL" in call(acc_weights=None)
    assert "invalid argument: acc_flags is NULL" in call(acc_flags=None)
    assert "input_flags is NULL" in call(mode=1)
    assert "input_flags is NULL" in call(mode=2)
    assert "input_flags given" in call(input_flags=p)
    assert "input_flags_mode" in call(mode=3, input_flags=p)
    assert "input_flags_mode" in call(mode=-1, input_flags=p)
    assert "channels" in call(channels=0)
    assert "baselines" in call(baselines=0)
    assert "invalid argument: vis" + small in call(vis_stride=7)
    assert "acc_vis" not in _lib.last_error()
    assert "invalid argument: flags" + small in call(flags_stride=7)
    assert "invalid argument: weights" + small in call(weights_stride=7)
    assert "invalid argument: input_flags" + small in call(
        mode=2, input_flags=p, input_flags_stride=7)  # fmt: skip
    assert "invalid argument: acc_vis" + small in call(acc_vis_stride=7)
    assert "invalid argument: acc_weights" + small in call(acc_weights_stride=7)
    assert "invalid argument: acc_flags" + small in call(acc_flags_stride=7)
    # the order of the checks: everything wrong at once, then only every stride
    strides = {name + "_stride": -1 for name in (
        "vis", "flags", "weights", "input_flags", "acc_vis", "acc_weights", "acc_flags")}  # fmt: skip
    assert "invalid argument: vis is NULL" in call(
        vis=None, flags=None, weights=None, acc_vis=None, acc_weights=None, acc_flags=None,
        channels=0, baselines=0, **strides)  # fmt: skip
    assert "invalid argument: vis" + small in call(mode=2, input_flags=p, **strides)


def test_finalise_argument_validation_without_gpu(lib):
    from katsdpsigproc_amd import _lib

    p = ctypes.c_void_p(64)  # never dereferenced: every call below fails its checks first

    def call(acc_vis=p, acc_weights=p, acc_flags=p, out_vis=p, out_weights=p, out_flags=p,
             channels=4, baselines=8, channel_factor=2, clear=1, acc_vis_stride=8,
             acc_weights_stride=8, acc_flags_stride=8, out_vis_stride=8, out_weights_stride=8,
             out_flags_stride=8):  # fmt: skip
        rc = lib.ksp_average_finalise(
            0, None, acc_vis, acc_weights, acc_flags, out_vis, out_weights, out_flags, channels,
            baselines, channel_factor, clear, acc_vis_stride, acc_weights_stride,
            acc_flags_stride, out_vis_stride, out_weights_stride, out_flags_stride)  # fmt: skip
        assert rc != 0
        return _lib.last_error()

    for name in ("acc_vis", "acc_weights", "acc_flags", "out_vis", "out_weights", "out_flags"):
        assert f"invalid argument: {name} is NULL" in call(**{name: None})
        assert f"invalid argument: {name}_stride is smaller than baselines" in call(
            **{name + "_stride": 7})  # fmt: skip
    assert "channels" in call(channels=0)
    assert "baselines" in call(baselines=0)
    assert "channel_factor must be" in call(channel_factor=0)
    assert "channel_factor does not divide" in call(channel_factor=3)
    # the order of the checks: everything wrong at once, then only every stride
    names = ("acc_vis", "acc_weights", "acc_flags", "out_vis", "out_weights", "out_flags")
    strides = {name + "_stride": -1 for name in names}
    assert "invalid argument: acc_vis is NULL" in call(
        **dict.fromkeys(names), channels=0, baselines=0, channel_factor=0, **strides)
    assert "invalid argument: acc_vis_stride is smaller than baselines" in call(**strides)
