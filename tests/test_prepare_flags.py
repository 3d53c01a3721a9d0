"""Static masks per baseline class and per-baseline flags in ``Prepare``, without a GPU:
``rfi.host.PrepareHost`` with `mask_index` and `baseline_flags` against known answers and a
triple loop of Python scalars, the new argument errors of the host class, template, operation
and adapter, slots and every launch argument of every new branch on the fake backend, the
sequence prepare -> fused flagger -> accumulate -> finalise, and the argument checks of
``ksp_prepare_flags``, which come before any device call."""

import ctypes

import numpy as np
import pytest

from katsdpsigproc_amd import accel
from katsdpsigproc_amd.rfi import device, host, ingest
from tests.fakes import FakeContext
from tests.test_prepare import LOST, arange32, loop_case, same_bits, triple_loop

FULL = device.BackgroundFlags.FULL
f32 = np.float32
u8 = np.uint8


@pytest.fixture
def context():
    return FakeContext()


@pytest.fixture
def queue(context):
    return context.create_command_queue()


def flags_of(vis_in, **kwargs):
    lost_flag = kwargs.pop("lost_flag", 8)
    vis, flags, weights = host.PrepareHost(lost_flag=lost_flag)(
        vis_in, arange32(vis_in.shape[1]), **kwargs)  # fmt: skip
    assert flags.dtype == u8 and flags.shape == vis.shape == vis_in.shape[:2]
    return flags


# ------------------------------------------------------------------------ known answers
def test_class_0_against_class_1():
    vis_in = np.ones((2, 3, 2), np.int32)
    masks = np.array([[0x01, 0x00], [0x02, 0x40]], u8)  # (classes, channels)
    flags = flags_of(vis_in, channel_flags=masks, mask_index=np.array([0, 1, 0], u8))
    assert flags.tolist() == [[0x01, 0x02, 0x01], [0x00, 0x40, 0x00]]
    assert host.PrepareHost.MAX_CLASSES == 8


@pytest.mark.parametrize("classes", [1, 2, 8])
def test_index_outside_the_classes_is_no_mask(classes):
    vis_in = np.ones((1, 4, 2), np.int32)
    masks = np.full((classes, 1), 0xFF, u8)
    index = np.array([classes - 1, classes, 255, 0], u8)
    flags = flags_of(vis_in, channel_flags=masks, mask_index=index)
    assert flags.tolist() == [[0xFF, 0, 0, 0xFF]]


def test_overlapping_bits_are_ored_not_added():
    vis_in = np.ones((1, 2, 2), np.int32)
    vis_in[0, 1, 0] = LOST
    flags = flags_of(vis_in, lost_flag=0x0C, channel_flags=np.array([[0x05]], u8),
                     mask_index=np.zeros(2, u8), baseline_flags=np.array([0x0D, 0x0D], u8))  # fmt: skip
    assert flags.tolist() == [[0x0D, 0x0D]]  # 0x05 | 0x0D (| 0x0C): a sum would be 0x12 (0x1E)


def test_lost_sample_on_a_flagged_baseline():
    vis_in = np.full((2, 2, 2), 7, np.int32)
    vis_in[1, 0, 0] = LOST
    prepare = host.PrepareHost(scale=0.5, lost_flag=0x08)
    source, auto = arange32(2), np.zeros((2, 2), np.int32)
    vis, flags, weights = prepare(vis_in, source, None, auto, np.array([0x80, 0], u8))
    assert flags.tolist() == [[0x80, 0], [0x88, 0]]
    # a baseline flagged so keeps its visibility and its weight
    plain = prepare(vis_in, source, None, auto)
    same_bits(plain[0], vis)
    same_bits(plain[2], weights)
    assert vis[0, 0] == 3.5 + 3.5j and vis[1, 0] == 0 and weights[0, 0] == f32(1 / 12.25)


def test_baseline_flags_without_channel_flags():
    vis_in = np.ones((3, 4, 2), np.int32)
    flags = flags_of(vis_in, baseline_flags=np.array([0, 0x21, 0, 0xFF], u8))
    assert flags.tolist() == [[0, 0x21, 0, 0xFF]] * 3


# ----------------------------------------------------------------------- the triple loop
def scalar_flags(lost, channel_flags, mask_index, baseline_flags, lost_flag):
    """The issue's formula for ``input_flags``, sample by sample, in Python ints; `lost` is
    channels x baselines."""
    channels, baselines = lost.shape
    out = np.zeros((channels, baselines), u8)
    for c in range(channels):
        for j in range(baselines):
            if mask_index is not None:
                k = int(mask_index[j])
                cf = int(channel_flags[k][c]) if k < len(channel_flags) else 0
            else:
                cf = int(channel_flags[c]) if channel_flags is not None else 0
            bf = int(baseline_flags[j]) if baseline_flags is not None else 0
            out[c, j] = cf | bf | (lost_flag if lost[c, j] else 0)
    return out


def flags_case(classes, seed=7):
    """What goes with loop_case(): masks that differ in every class and channel, indices from
    0 .. classes + 1 and 255, baseline flags that are zero on about half the baselines."""
    rs = np.random.RandomState(seed + classes)
    masks = rs.randint(0, 256, (classes, 5)).astype(u8)
    index = rs.choice(list(range(classes + 2)) + [255], 9).astype(u8)
    index[:3] = [classes, 255, classes - 1]
    baseline_flags = np.where(rs.random_sample(9) < 0.5, rs.randint(1, 256, 9), 0).astype(u8)
    baseline_flags[:2] = [0, 0x29]  # (0x29 overlaps the lost_flag of the test, 0x28)
    return masks, index, baseline_flags


@pytest.mark.parametrize("classes", [1, 2, 3, 8])
@pytest.mark.parametrize("use_baseline_flags", [False, True])
@pytest.mark.parametrize("use_weights", [False, True])
def test_host_against_triple_loop(use_weights, use_baseline_flags, classes):
    vis_in, source, _, auto_source = loop_case()
    masks, index, baseline_flags = flags_case(classes)
    assert (index >= classes).any() and (index == 255).any() and (index < classes).any()
    auto_source = auto_source if use_weights else None
    baseline_flags = baseline_flags if use_baseline_flags else None
    got = host.PrepareHost(1.0 / 3.0, 0x28, 7.0)(
        vis_in, source, masks, auto_source, baseline_flags=baseline_flags, mask_index=index)
    plain = triple_loop(vis_in, source, None, auto_source, 1.0 / 3.0, 0x28, 7.0)
    lost = plain[1] != 0
    assert lost.any() and not lost.all()
    same_bits(plain[0], got[0])
    same_bits(scalar_flags(lost, masks, index, baseline_flags, 0x28), got[1])
    if use_weights:
        same_bits(plain[2], got[2])
    else:
        assert got[2] is None


@pytest.mark.parametrize("use_channel_flags", [False, True])
@pytest.mark.parametrize("use_weights", [False, True])
def test_without_the_new_arguments_nothing_changes(use_weights, use_channel_flags):
    vis_in, source, channel_flags, auto_source = loop_case()
    channel_flags = channel_flags if use_channel_flags else None
    auto_source = auto_source if use_weights else None
    prepare = host.PrepareHost(2.0**-8, 0x28, 2.0**20)
    want = triple_loop(vis_in, source, channel_flags, auto_source, 2.0**-8, 0x28, 2.0**20)
    for got in (prepare(vis_in, source, channel_flags, auto_source),
                prepare(vis_in, source, channel_flags, auto_source, None, None),
                prepare(vis_in, source, channel_flags, auto_source, baseline_flags=np.zeros(9, u8))):  # fmt: skip
        for w, g in zip(want, got):
            if w is None:
                assert g is None
            else:
                same_bits(w, g)
    # one class that every baseline has is the single row of before
    if use_channel_flags:
        got = prepare(vis_in, source, channel_flags[np.newaxis], auto_source,
                      mask_index=np.zeros(9, u8))  # fmt: skip
        same_bits(want[1], got[1])


# ------------------------------------------------------------------------------- errors
def test_host_errors():
    prepare = host.PrepareHost()
    vis_in = np.zeros((4, 6, 2), np.int32)
    good = {"vis_in": vis_in, "source": arange32(5), "channel_flags": np.zeros((2, 4), u8),
            "auto_source": np.zeros((5, 2), np.int32), "baseline_flags": np.zeros(5, u8),
            "mask_index": np.zeros(5, u8)}  # fmt: skip
    prepare(**good)
    for name, bad in [
        ("mask_index", np.zeros(5, np.int32)), ("mask_index", np.zeros(5, np.int8)),
        ("mask_index", np.zeros(4, u8)), ("mask_index", np.zeros((5, 1), u8)),
        ("mask_index", np.zeros((1, 5), u8)),
        ("baseline_flags", np.zeros(5, bool)), ("baseline_flags", np.zeros(5, np.int32)),
        ("baseline_flags", np.zeros(6, u8)), ("baseline_flags", np.zeros((5, 1), u8)),
        ("baseline_flags", np.zeros((), u8)),
        # with mask_index: (classes, channels), 1 .. 8 classes
        ("channel_flags", np.zeros(4, u8)), ("channel_flags", np.zeros((2, 5), u8)),
        ("channel_flags", np.zeros((4, 2), u8)), ("channel_flags", np.zeros((0, 4), u8)),
        ("channel_flags", np.zeros((9, 4), u8)), ("channel_flags", np.zeros((2, 4), np.int8)),
        ("channel_flags", np.zeros((1, 2, 4), u8)), ("channel_flags", None),
    ]:  # fmt: skip
        with pytest.raises(ValueError, match=name):
            prepare(**{**good, name: bad})
    # and the reverse: classes without an index
    with pytest.raises(ValueError, match="channel_flags"):
        prepare(**{**good, "mask_index": None})
    prepare(**{**good, "channel_flags": np.zeros((8, 4), u8)})
    prepare(**{**good, "channel_flags": np.zeros(4, u8), "mask_index": None})


def test_template_and_operation_errors(context, queue):
    for bad in (9, -1, 256):
        with pytest.raises(ValueError, match="mask_classes"):
            ingest.PrepareTemplate(context, channel_flags=True, mask_classes=bad)
    for classes in range(1, 9):
        with pytest.raises(ValueError, match="channel_flags"):
            ingest.PrepareTemplate(context, mask_classes=classes)
        with pytest.raises(ValueError, match="channel_flags"):
            ingest.PrepareTemplate(context, mask_classes=classes, baseline_flags=True)
        template = ingest.PrepareTemplate(context, channel_flags=True, mask_classes=classes)
        assert template.mask_classes == classes and template.kernel.name == "ksp_prepare_flags"
    with pytest.raises(ValueError):
        ingest.PrepareTemplate(context, baseline_flags=True, tuning={"wgs": 256})
    template = ingest.PrepareTemplate(context, baseline_flags=True)
    assert template.mask_classes == 0 and template.baseline_flags is True
    assert ingest.PrepareTemplate.KERNEL == "ksp_prepare"
    assert ingest.PrepareTemplate(context, channel_flags=True).kernel.name == "ksp_prepare"
    for args in [(0, 4), (4, 0), (4, 4, 0)]:
        with pytest.raises(ValueError):
            template.instantiate(queue, *args)


def test_host_from_device_errors(context, queue):
    vis_in = np.zeros((4, 6, 2), np.int32)
    source = arange32(5)
    masks, row = np.zeros((2, 4), u8), np.zeros(4, u8)
    per_baseline = np.zeros(5, u8)
    plain = ingest.PrepareHostFromDevice(ingest.PrepareTemplate(context, channel_flags=True), queue)
    with pytest.raises(TypeError, match="baseline_flags"):
        plain(vis_in, source, row, baseline_flags=per_baseline)
    with pytest.raises(TypeError, match="mask_index"):
        plain(vis_in, source, masks, mask_index=per_baseline)
    both = ingest.PrepareHostFromDevice(
        ingest.PrepareTemplate(context, channel_flags=True, mask_classes=2, baseline_flags=True),
        queue)  # fmt: skip
    with pytest.raises(TypeError, match="baseline_flags"):
        both(vis_in, source, masks, mask_index=per_baseline)
    with pytest.raises(TypeError, match="mask_index"):
        both(vis_in, source, masks, baseline_flags=per_baseline)
    with pytest.raises(TypeError, match="channel_flags"):
        both(vis_in, source, baseline_flags=per_baseline, mask_index=per_baseline)
    for wrong in (row, np.zeros((3, 4), u8), np.zeros((1, 4), u8)):
        with pytest.raises(ValueError, match="channel_flags"):
            both(vis_in, source, wrong, baseline_flags=per_baseline, mask_index=per_baseline)
    assert not queue.launches
    vis, flags, weights = both(vis_in, source, masks, None, per_baseline, per_baseline)
    assert vis.shape == flags.shape == (4, 5) and weights is None
    only = ingest.PrepareHostFromDevice(ingest.PrepareTemplate(context, baseline_flags=True), queue)
    assert only(vis_in, source, baseline_flags=per_baseline)[1].shape == (4, 5)
    plain(vis_in, source, row)
    assert [name for name, _ in queue.launches] == ["ksp_prepare_flags"] * 2 + ["ksp_prepare"]
    assert [int(a) for a in queue.launches[0][1][9:13]] == [4, 6, 5, 2]


# ------------------------------------------------------------------------------- wiring
BRANCHES = [(0, True, False), (0, True, True), (1, False, True), (1, True, True),
            (2, False, True), (3, True, True), (8, False, True), (8, True, True)]  # fmt: skip


@pytest.mark.parametrize("classes, use_baseline_flags, use_channel_flags", BRANCHES)
@pytest.mark.parametrize("use_weights", [False, True])
def test_wiring(use_weights, classes, use_baseline_flags, use_channel_flags, context, queue):
    template = ingest.PrepareTemplate(context, scale=0.1, lost_flag=0x40,
                                      channel_flags=use_channel_flags, weights=use_weights,
                                      weight_scale=3.0, mask_classes=classes,
                                      baseline_flags=use_baseline_flags)  # fmt: skip
    fn = template.instantiate(queue, 300, 200, 250)
    shapes = {"vis_in": (300, 250, 2), "source": (200,), "vis": (300, 200),
              "input_flags": (300, 200)}  # fmt: skip
    if use_channel_flags:
        shapes["channel_flags"] = (classes, 300) if classes else (300,)
    if classes:
        shapes["mask_index"] = (200,)
    if use_baseline_flags:
        shapes["baseline_flags"] = (200,)
    if use_weights:
        shapes.update({"auto_source": (200, 2), "weights": (300, 200)})
    dtypes = {"vis_in": np.int32, "source": np.int32, "auto_source": np.int32,
              "vis": np.complex64, "weights": np.float32}  # fmt: skip
    assert set(fn.slots) == set(shapes)
    for name, shape in shapes.items():
        assert fn.slots[name].shape == shape and fn.slots[name].dtype == dtypes.get(name, u8)
    # the classes are never padded apart, the channels of a class can be
    if classes:
        assert fn.slots["channel_flags"].dimensions[0].exact
        assert not fn.slots["channel_flags"].dimensions[1].exact
    # a dimension object of its own for everything that can be padded
    dims = [d for slot in fn.slots.values() for d in slot.dimensions]
    assert len({id(d) for d in dims}) == len(dims)
    accel.Dimension(200, min_padded_size=500).link(fn.slots["input_flags"].dimensions[1])
    if classes:
        accel.Dimension(300, min_padded_size=333).link(fn.slots["channel_flags"].dimensions[1])
    fn()
    assert [name for name, _ in queue.launches] == ["ksp_prepare_flags"]
    args = queue.launches[0][1]
    assert len(args) == 21

    def buffer_of(name, there=True):
        return fn.buffer(name).buffer if there else None

    assert args[0] is buffer_of("vis_in") and args[1] is buffer_of("source")
    assert args[2] is buffer_of("auto_source", use_weights)
    assert args[3] is buffer_of("channel_flags", use_channel_flags)
    assert args[4] is buffer_of("mask_index", classes)
    assert args[5] is buffer_of("baseline_flags", use_baseline_flags)
    assert args[6] is buffer_of("vis") and args[7] is buffer_of("input_flags")
    assert args[8] is buffer_of("weights", use_weights)
    assert all(isinstance(a, np.int32) for a in args[9:18]) and isinstance(args[20], np.int32)
    assert [int(a) for a in args[9:13]] == [300, 250, 200, classes]

    def padded(name):
        return fn.buffer(name).padded_shape

    assert [int(a) for a in args[13:18]] == [
        padded("vis_in")[1], padded("channel_flags")[1] if classes else 0, padded("vis")[1],
        padded("input_flags")[1], padded("weights")[1] if use_weights else 0]  # fmt: skip
    if classes:
        assert padded("channel_flags")[0] == classes and padded("channel_flags")[1] >= 333
    assert padded("input_flags")[1] == 512
    assert isinstance(args[18], np.float32) and args[18] == f32(0.1)
    assert isinstance(args[19], np.float32) and args[19] == f32(3.0)
    assert int(args[20]) == 0x40
    want = {"scale": float(f32(0.1)), "lost_flag": 0x40, "channel_flags": use_channel_flags,
            "weights": use_weights, "weight_scale": 3.0, "in_baselines": 250, "channels": 300,
            "baselines": 200}  # fmt: skip
    if classes:
        want["mask_classes"] = classes
    if use_baseline_flags:
        want["baseline_flags"] = True
    assert fn.parameters() == want


@pytest.mark.parametrize("use_channel_flags", [False, True])
@pytest.mark.parametrize("use_weights", [False, True])
def test_options_off_is_the_old_launch(use_weights, use_channel_flags, context, queue):
    template = ingest.PrepareTemplate(context, channel_flags=use_channel_flags,
                                      weights=use_weights, mask_classes=0, baseline_flags=False)  # fmt: skip
    fn = template.instantiate(queue, 30, 20)
    assert not {"mask_index", "baseline_flags"} & set(fn.slots)
    fn()
    assert [name for name, _ in queue.launches] == ["ksp_prepare"]
    assert len(queue.launches[0][1]) == 17
    assert set(fn.parameters()) == {"scale", "lost_flag", "channel_flags", "weights",
                                    "weight_scale", "in_baselines", "channels", "baselines"}  # fmt: skip


def test_in_front_of_the_chain(context, queue):
    """prepare (2 classes, baseline flags, weights) -> fused flagger (FULL) -> accumulate
    (weights, FULL) -> finalise: `input_flags` is one buffer with one padded size."""
    channels, baselines, in_baselines = 4096, 200, 260
    prepare = ingest.PrepareTemplate(context, weights=True, channel_flags=True, mask_classes=2,
                                     baseline_flags=True).instantiate(
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
    accel.Dimension(baselines, min_padded_size=400).link(accumulate.slots["input_flags"].dimensions[1])
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
    assert {"prepare:vis_in", "prepare:source", "prepare:auto_source", "prepare:channel_flags",
            "prepare:mask_index", "prepare:baseline_flags"} <= set(seq.slots)  # fmt: skip
    assert "prepare:input_flags" not in seq.slots
    for name in device.FusedFlaggerDevice._OPTIONAL:
        del seq.slots["flagger:" + name]
    seq()
    assert [name for name, _ in queue.launches] == [
        "ksp_prepare_flags", "ksp_flagger_fused", "ksp_average_accumulate",
        "ksp_average_finalise"]  # fmt: skip
    prep_args, flag_args, add_args, _ = (launch[1] for launch in queue.launches)
    assert prepare.buffer("input_flags") is flagger.buffer("input_flags")
    assert prepare.buffer("input_flags") is accumulate.buffer("input_flags")
    assert prepare.buffer("input_flags") is seq.buffer("input_flags")
    assert prep_args[6] is flag_args[0] is add_args[0] is seq.buffer("vis").buffer
    assert prep_args[7] is flag_args[1] is add_args[3] is seq.buffer("input_flags").buffer
    assert prep_args[8] is add_args[2] is seq.buffer("weights").buffer
    assert prep_args[4] is seq.buffer("prepare:mask_index").buffer
    assert prep_args[5] is seq.buffer("prepare:baseline_flags").buffer
    mask_stride = seq.buffer("input_flags").padded_shape[1]
    assert mask_stride == 512  # 400 rounded up to whole 128-byte rows
    assert int(prep_args[16]) == int(flag_args[8]) == int(add_args[13]) == mask_stride
    assert int(prep_args[15]) == int(flag_args[7]) == int(add_args[10])
    assert int(prep_args[12]) == 2
    assert int(prep_args[14]) == seq.buffer("prepare:channel_flags").padded_shape[1] >= channels


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

    def call(vis_in=p, source=p, auto_source=p, channel_flags=p, mask_index=p, baseline_flags=p,
             vis=p, input_flags=p, weights=p, channels=4, in_baselines=8, baselines=8,
             mask_classes=2, vis_in_stride=8, channel_flags_stride=4, vis_stride=8,
             input_flags_stride=8, weights_stride=8, scale=1.0, weight_scale=1.0, lost_flag=8):  # fmt: skip
        rc = lib.ksp_prepare_flags(
            0, None, vis_in, source, auto_source, channel_flags, mask_index, baseline_flags, vis,
            input_flags, weights, channels, in_baselines, baselines, mask_classes, vis_in_stride,
            channel_flags_stride, vis_stride, input_flags_stride, weights_stride, scale,
            weight_scale, lost_flag)  # fmt: skip
        assert rc != 0
        return _lib.last_error()

    assert "invalid argument: vis_in is NULL" in call(vis_in=None)
    assert "invalid argument: source is NULL" in call(source=None)
    assert "invalid argument: vis is NULL" in call(vis=None)
    assert "invalid argument: input_flags is NULL" in call(input_flags=None)
    assert "auto_source and weights must both" in call(auto_source=None)
    assert "auto_source and weights must both" in call(weights=None)
    for bad in (-1, 9, 256):
        assert "mask_classes must be 0..8" in call(mask_classes=bad)
    assert "mask_index must be given exactly when" in call(mask_index=None)
    assert "mask_index must be given exactly when" in call(mask_classes=0)
    for classes in (1, 8):
        assert "need channel_flags" in call(channel_flags=None, mask_classes=classes)
    assert "channels must be" in call(channels=0)
    assert "in_baselines must be" in call(in_baselines=0)
    assert "invalid argument: baselines must be" in call(baselines=0)
    assert "invalid argument: vis_in_stride is smaller than in_baselines" in call(vis_in_stride=7)
    assert "invalid argument: channel_flags_stride is smaller than channels" in call(
        channel_flags_stride=3)  # fmt: skip
    for name in ("vis", "input_flags", "weights"):
        assert f"invalid argument: {name}_stride is smaller than baselines" in call(
            **{name + "_stride": 7})  # fmt: skip
    # the order of the checks: everything wrong at once, then only every stride
    strides = dict(vis_in_stride=-1, channel_flags_stride=-1, vis_stride=-1,
                   input_flags_stride=-1, weights_stride=-1)  # fmt: skip
    assert "invalid argument: vis_in is NULL" in call(
        vis_in=None, source=None, auto_source=None, channel_flags=None, mask_index=None,
        baseline_flags=None, vis=None, input_flags=None, weights=None, channels=0,
        in_baselines=0, baselines=0, **strides)  # fmt: skip
    assert "invalid argument: vis_in_stride is smaller than in_baselines" in call(**strides)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert "invalid argument: scale must be finite" in call(scale=bad)
        assert "weight_scale must be finite" in call(weight_scale=bad)
    for bad in (0, 256, -8):
        assert "lost_flag must be 1..255" in call(lost_flag=bad)
    # without classes the row stride of channel_flags is not looked at, with or without a row,
    # and what belongs to the weights is not looked at without them
    for row in (p, None):
        message = call(channel_flags=row, mask_index=None, mask_classes=0,
                       channel_flags_stride=0, auto_source=None, weights=None, weights_stride=0,
                       weight_scale=0.0, lost_flag=0)  # fmt: skip
        assert "lost_flag" in message
    assert "lost_flag" in call(baseline_flags=None, lost_flag=0)
    assert "too large for one launch" in call(
        channels=2**31 - 1, in_baselines=1, baselines=2**31 - 1, vis_in_stride=1,
        channel_flags_stride=2**31 - 1, vis_stride=2**31 - 1, input_flags_stride=2**31 - 1,
        weights_stride=2**31 - 1)  # fmt: skip
