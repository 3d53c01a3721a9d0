"""Static masks per baseline class and per-baseline flags of ``Prepare`` on the GPU
(``rfi.ingest.PrepareTemplate(mask_classes=..., baseline_flags=...)``, ``ksp_prepare_flags``):
every comparison is of bit patterns, against ``rfi.host.PrepareHost``, with nothing left out."""

import ctypes

import numpy as np
import pytest

from tests import inputs
from tests.subviews import SENTINEL, CompactViews, flat_device_array, sentinel_array
from tests.test_gpu_prepare import (N_AUTO, assert_same, chain_dump, make_case, read_checked,
                                    write_padded)  # fmt: skip

pytestmark = pytest.mark.gpu

u8 = np.uint8
# A lane owns a run of 16 baselines: a ragged last run, one full run, a full run and a ragged
# one, two full runs, and a wavefront's (1024) and more than a workgroup's worth of rows' runs.
BASELINES = [1, 3, 15, 16, 17, 31, 32, 33, 257, 1025]
# ... of 4 adjacent rows with weights and 2 without: every remainder of both.
CHANNELS = [1, 2, 3, 4, 5, 9]
CLASSES = [0, 1, 2, 3, 8]  # 0: the single row of channel flags without mask_index
NO_CHANNEL_FLAGS = -1  # in place of a number of classes: no channel flags at all


@pytest.fixture(scope="module")
def context():
    from katsdpsigproc_amd import accel

    return accel.create_some_context(interactive=False)


@pytest.fixture(scope="module")
def command_queue(context):
    return context.create_command_queue()


def make_flags(seed, channels, baselines, classes):
    """(masks, mask_index, baseline_flags): masks (max(classes, 1), channels) whose bytes all
    differ, so that a wrong class or a wrong row shows; indices from 0 .. classes + 1 and 255
    (``None`` without classes); baseline flags that are zero on about half the baselines."""
    rs = np.random.RandomState(seed)
    k, c = np.meshgrid(np.arange(max(classes, 1)), np.arange(channels), indexing="ij")
    masks = (1 + 31 * k + 3 * (c % 10)).astype(u8)
    index = None
    if classes >= 1:
        index = rs.choice(list(range(classes + 2)) + [255], baselines).astype(u8)
        first = np.array([classes, 255, classes - 1, 0], u8)[:baselines]
        index[-len(first) :] = first  # (the end of the row: its last, perhaps ragged, run)
    baseline_flags = np.where(rs.random_sample(baselines) < 0.5,
                              rs.randint(1, 256, baselines), 0).astype(u8)  # fmt: skip
    return masks, index, baseline_flags


def host_arguments(case, flags, classes, use_baseline_flags, use_weights):
    """The arguments of PrepareHost (and of the adapter) for one variant."""
    vis_in, source, _, auto_source = case
    masks, index, baseline_flags = flags
    masks = None if classes == NO_CHANNEL_FLAGS else masks if classes else masks[0]
    return (vis_in, source, masks, auto_source if use_weights else None,
            baseline_flags if use_baseline_flags else None, index if classes >= 1 else None)  # fmt: skip


def write_filled(queue, array, data, fill=0xFF):
    """`data` into `array`, `fill` bytes into its padding."""
    raw = np.full(array.padded_shape, fill, array.dtype)
    raw[tuple(slice(0, n) for n in array.shape)] = data
    queue.enqueue_write_buffer(array.buffer, raw)


def run_device(context, queue, arguments, classes, scale, lost_flag, weight_scale, pad=0):
    """(vis, input_flags, weights or None) of the operation with a single row of channel flags
    (`classes` 0), `classes` rows or none (NO_CHANNEL_FLAGS). The outputs start out full of
    sentinel bytes, padding included, and every padding is checked afterwards; the padding of
    the rows of `channel_flags` and of the per-baseline inputs holds 0xFF."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import ingest

    vis_in, source, masks, auto_source, baseline_flags, index = arguments
    use_weights, use_baseline_flags = auto_source is not None, baseline_flags is not None
    channels, in_baselines = vis_in.shape[:2]
    template = ingest.PrepareTemplate(context, scale, lost_flag, masks is not None, use_weights,
                                      weight_scale, mask_classes=max(classes, 0),
                                      baseline_flags=use_baseline_flags)  # fmt: skip
    assert template.kernel.name == "ksp_prepare_flags"
    fn = template.instantiate(queue, channels, len(source), in_baselines)
    if pad:
        for name in ("vis_in", "vis", "input_flags", "weights", "channel_flags"):
            if name in fn.slots and len(fn.slots[name].dimensions) >= 2:
                dim = fn.slots[name].dimensions[1]
                accel.Dimension(dim.size, min_padded_size=dim.size + pad).link(dim)
    fn.ensure_all_bound()
    outputs = ["vis", "input_flags"] + (["weights"] if use_weights else [])
    for name in outputs:
        assert fn.buffer(name).padded_shape[1] >= len(source) + pad
        write_padded(queue, fn.buffer(name), sentinel_array((1,), fn.buffer(name).dtype)[0])
    write_padded(queue, fn.buffer("vis_in"), vis_in)
    fn.buffer("source").set(queue, source)
    if masks is not None:
        write_filled(queue, fn.buffer("channel_flags"), masks)
    if classes >= 1:
        assert fn.buffer("channel_flags").padded_shape[0] == classes
        assert fn.buffer("channel_flags").padded_shape[1] >= channels + pad
        write_filled(queue, fn.buffer("mask_index"), index)
    if use_baseline_flags:
        write_filled(queue, fn.buffer("baseline_flags"), baseline_flags)
    if use_weights:
        fn.buffer("auto_source").set(queue, auto_source)
    fn()
    got = [read_checked(queue, fn.buffer(name), name) for name in outputs]
    return got[0], got[1], (got[2] if use_weights else None)


def compare(context, queue, case, flags, classes, use_baseline_flags, use_weights, what,
            scale=2.0**-8, lost_flag=8, weight_scale=2.0**20, pad=0):  # fmt: skip
    from katsdpsigproc_amd.rfi import host

    arguments = host_arguments(case, flags, classes, use_baseline_flags, use_weights)
    want = host.PrepareHost(scale, lost_flag, weight_scale)(*arguments)
    got = run_device(context, queue, arguments, classes, scale, lost_flag, weight_scale, pad)
    what = f"{what}, {classes} classes, baseline flags {use_baseline_flags}, weights {use_weights}"
    for name, w, g in zip(("vis", "input_flags", "weights"), want, got):
        if w is None:
            assert g is None
        else:
            assert_same(w, g, f"{name} {what}")
    return want


def variants():
    """(classes, baseline flags) of every new instance: not (0, False), which is ksp_prepare."""
    with_masks = [(k, bf) for k in CLASSES for bf in (False, True) if k or bf]
    return [(NO_CHANNEL_FLAGS, True)] + with_masks


def test_data_covers_the_cases():
    from katsdpsigproc_amd.rfi import host

    case = make_case(1, 9, 257, 262, "permutation")
    assert 0.03 < np.mean(case[0][..., 0] == -(2**31)) < 0.08
    for classes in CLASSES[1:]:
        masks, index, baseline_flags = make_flags(classes, 9, 257, classes)
        assert len(np.unique(masks)) == masks.size == 9 * classes and masks.all()
        assert (index == classes).any() and (index == classes + 1).any() and (index == 255).any()
        assert all((index == k).any() for k in range(classes))
        assert 0.35 < np.mean(baseline_flags == 0) < 0.65
        arguments = host_arguments(case, (masks, index, baseline_flags), classes, True, False)
        flags = host.PrepareHost(lost_flag=8)(*arguments)[1]
        none = index >= classes
        assert np.all(flags[:, none] & ~(baseline_flags[none] | u8(8)) == 0)
    masks, index, _ = make_flags(1, 1, 1, 8)
    assert index.tolist() == [8]


@pytest.mark.parametrize("use_weights", [False, True])
@pytest.mark.parametrize("channels", CHANNELS)
def test_shapes(channels, use_weights, context, command_queue):
    """Every width and height with every new instance and number of classes."""
    rs = np.random.RandomState(channels)
    for baselines in BASELINES:
        in_baselines = [1, baselines, baselines + 5, 2 * baselines][rs.randint(4)]
        case = make_case(channels * 10007 + baselines, channels, baselines, in_baselines,
                         "permutation")  # fmt: skip
        for classes, use_baseline_flags in variants():
            flags = make_flags(baselines + classes, channels, baselines, classes)
            compare(context, command_queue, case, flags, classes, use_baseline_flags, use_weights,
                    f"{channels}x{baselines} from {in_baselines}",
                    lost_flag=[8, 0x81][rs.randint(2)])  # fmt: skip


@pytest.mark.parametrize("use_weights", [False, True])
@pytest.mark.parametrize("channels, baselines, pad", [(9, 33, 29), (5, 257, 3), (3, 32, 16)])
def test_padding(channels, baselines, pad, use_weights, context, command_queue):
    """Rows padded beyond what the slots ask for, those of `channel_flags` as well, whose
    padding holds 0xFF; run_device looks at the sentinels in the padding of all outputs."""
    case = make_case(pad, channels, baselines, baselines + 5, "permutation")
    for classes, use_baseline_flags in [(NO_CHANNEL_FLAGS, True), (0, True), (1, False), (2, True),
                                        (8, True)]:  # fmt: skip
        flags = make_flags(pad + classes, channels, baselines, classes)
        compare(context, command_queue, case, flags, classes, use_baseline_flags, use_weights,
                f"pad {pad}", pad=pad)  # fmt: skip


ALIGNED_STRIDES = {"vis_in": 24, "vis": 42, "input_flags": 48, "weights": 44}
ODD_STRIDES = {"vis_in": 23, "vis": 41, "input_flags": 39, "weights": 43}


@pytest.mark.parametrize("use_weights", [False, True])
@pytest.mark.parametrize("classes, use_baseline_flags", [(0, True), (2, True), (3, False)])
@pytest.mark.parametrize("flag_offset, offset, strides", [
    (1, 1, ODD_STRIDES), (4, 4, ODD_STRIDES), (1, 16, ALIGNED_STRIDES),
    (4, 16, ALIGNED_STRIDES), (16, 16, ALIGNED_STRIDES)])  # fmt: skip
def test_raw_abi_subviews(flag_offset, offset, strides, classes, use_baseline_flags, use_weights,
                          context, command_queue):  # fmt: skip
    """Sub-views: `mask_index` and `baseline_flags` `flag_offset` bytes into their
    allocations (1 and 4: the element-wise path, even where everything else is aligned; 16
    with everything else aligned: the 16-byte path from the middle of an allocation), the
    other arrays `offset` elements into theirs, a stride of its own per array and an odd one
    for the rows of `channel_flags`. 37 baselines: two whole runs and a ragged one, with
    indices outside the input and outside the classes in the last baselines."""
    check_raw_abi(flag_offset, offset, strides, classes, use_baseline_flags, use_weights,
                  context, command_queue)  # fmt: skip


def check_raw_abi(flag_offset, offset, strides, classes, use_baseline_flags, use_weights,
                  context, command_queue, views=None):  # fmt: skip
    """`views` makes the strided arrays (tests/subviews.py: CompactViews unless given) and may
    choose other strides of the same kind."""
    from katsdpsigproc_amd import _lib
    from katsdpsigproc_amd.rfi import host

    queue = command_queue
    views = views or CompactViews(context, queue)
    channels, in_baselines, baselines = 6, 21, 37
    # vis_in as rows of int32: a pair stride of n is a row stride of 2 n words; the rows of
    # channel_flags have an odd stride, 7
    strides = dict(strides, vis_in=2 * strides["vis_in"], channel_flags=channels + 1)

    def make(name, dtype, data, poison=False):
        """(view, pointer); the stride the launcher gets is the one the view was made with"""
        made = views(name, dtype, data, strides[name], offset, poison)
        strides[name] = made[0].stride
        return made

    case = list(make_case(offset, channels, baselines, in_baselines, "permutation"))
    case[1][-1] = in_baselines
    case[3][-1] = [-1, 2**31 - 1]
    flags = make_flags(flag_offset, channels, baselines, classes)
    arguments = host_arguments(case, flags, classes, use_baseline_flags, use_weights)
    vis_in, source, masks, _, _, _ = arguments
    auto_source, (_, index, baseline_flags) = case[3], flags
    d_in = make("vis_in", np.int32, vis_in.reshape(channels, -1), poison=True)
    assert strides["vis_in"] % 2 == 0
    d_source = flat_device_array(context, queue, np.int32, source[np.newaxis, :], baselines,
                                 offset, poison=True)  # fmt: skip
    d_auto = flat_device_array(context, queue, np.int32, auto_source.reshape(1, -1),
                               2 * baselines, offset, poison=True)  # fmt: skip
    d_masks = make("channel_flags", u8, np.atleast_2d(masks), poison=True)
    d_index = flat_device_array(context, queue, u8, (index if classes else baseline_flags)[np.newaxis, :],
                                baselines, flag_offset, poison=True)  # fmt: skip
    d_flags = flat_device_array(context, queue, u8, baseline_flags[np.newaxis, :], baselines,
                                flag_offset, poison=True)  # fmt: skip
    dtypes = {"vis": np.complex64, "input_flags": u8, "weights": np.float32}
    out = {name: make(name, dtype, sentinel_array((channels, baselines), dtype))
           for name, dtype in dtypes.items()}  # fmt: skip
    null = ctypes.c_void_p(0)
    _lib.call("ksp_prepare_flags", context.device.index, ctypes.c_void_p(queue.stream), d_in[1],
              d_source[1], d_auto[1] if use_weights else null, d_masks[1],
              d_index[1] if classes else null, d_flags[1] if use_baseline_flags else null,
              out["vis"][1], out["input_flags"][1], out["weights"][1] if use_weights else null,
              channels, in_baselines, baselines, classes, strides["vis_in"] // 2,
              strides["channel_flags"] if classes else 0, strides["vis"], strides["input_flags"],
              strides["weights"], 2.0**-8, 2.0**20, 0x10)  # fmt: skip
    want = host.PrepareHost(2.0**-8, 0x10, 2.0**20)(*arguments)
    for name, w in zip(dtypes, want):
        got = out[name][0].read(name)
        if w is None:  # no weights: nothing at all was written to that allocation
            assert np.all(got.view(u8) == SENTINEL)
        else:
            assert_same(w, got, f"{name} at offsets {offset} and {flag_offset}")
    for view in (d_in, d_source, d_auto, d_masks, d_index, d_flags):
        view[0].read("an input")  # (asserts that nothing wrote to it)


def test_host_from_device(context, command_queue):
    """The adapter with all options, and with each alone."""
    from katsdpsigproc_amd.rfi import host, ingest

    case = make_case(11, 12, 70, 90, "permutation")
    for classes, use_baseline_flags, use_weights in [(3, True, True), (2, False, False),
                                                     (0, True, False), (8, True, True)]:  # fmt: skip
        flags = make_flags(classes, 12, 70, classes)
        template = ingest.PrepareTemplate(context, 2.0**-8, 0x40, True, use_weights, 2.0**20,
                                          mask_classes=classes, baseline_flags=use_baseline_flags)  # fmt: skip
        arguments = host_arguments(case, flags, classes, use_baseline_flags, use_weights)
        got = ingest.PrepareHostFromDevice(template, command_queue)(*arguments)
        want = host.PrepareHost(2.0**-8, 0x40, 2.0**20)(*arguments)
        assert (got[2] is None) == (not use_weights)
        for name, w, g in zip(("vis", "input_flags", "weights"), want, got):
            if w is not None:
                assert_same(w, g, name)
    # baseline flags with no channel flags at all
    template = ingest.PrepareTemplate(context, 2.0**-8, 0x40, baseline_flags=True)
    vis_in, source = case[:2]
    got = ingest.PrepareHostFromDevice(template, command_queue)(vis_in, source, baseline_flags=flags[2])
    want = host.PrepareHost(2.0**-8, 0x40)(vis_in, source, baseline_flags=flags[2])
    assert_same(want[0], got[0], "vis")
    assert_same(want[1], got[1], "input_flags")


# (the host's noise estimate says so of the baseline whose every sample is flagged)
@pytest.mark.filterwarnings("ignore:baseline with no non-zero deviations")
def test_in_front_of_the_chain(context, command_queue):
    """Three dumps through prepare -> fused flagger -> accumulate -> finalise in one sequence
    against PrepareHost + FlaggerHost + AveragerHost: two classes of static mask, one baseline
    that `baseline_flags` flags in every dump and one that it flags in one dump only."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import device, host, ingest

    queue = command_queue
    channels, baselines, in_baselines, cf = 64, 40, 50, 4
    full = device.BackgroundFlags.FULL
    scale, lost_flag, weight_scale = 2.0**-8, 0x08, 2.0**24
    always, once, off_target = 5, 35, 0x40
    prepare = ingest.PrepareTemplate(context, scale, lost_flag, True, True, weight_scale,
                                     mask_classes=2, baseline_flags=True).instantiate(
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
    acc = ("acc_vis", "acc_weights", "acc_flags")
    compounds = {
        "vis": ["prepare:vis", "flagger:vis", "accumulate:vis"],
        "input_flags": ["prepare:input_flags", "flagger:input_flags", "accumulate:input_flags"],
        "weights": ["prepare:weights", "accumulate:weights"],
        "flags": ["flagger:flags", "accumulate:flags"],
    }
    compounds.update({name: ["accumulate:" + name, "finalise:" + name] for name in acc})
    seq = accel.OperationSequence(
        queue, [("prepare", prepare), ("flagger", flagger), ("accumulate", accumulate),
                ("finalise", finalise)], compounds=compounds)  # fmt: skip
    for name in device.FusedFlaggerDevice._OPTIONAL:
        del seq.slots["flagger:" + name]
    seq.ensure_all_bound()
    for name in acc:
        seq.buffer(name).zero(queue)
    rs = np.random.RandomState(9)
    source = rs.permutation(in_baselines)[:baselines].astype(np.int32)
    auto_source = rs.randint(0, N_AUTO, (baselines, 2)).astype(np.int32)
    # class 0: an eighth of the band, for baselines 10 .. 29; class 1: another eighth, for the
    # first 10 baselines only; the long baselines from 30 on have no static mask
    masks = np.stack([inputs.channel_mask(channels, seed=4, fraction=1.0 / 8.0) * u8(0x20),
                      inputs.channel_mask(channels, seed=5, fraction=1.0 / 8.0) * u8(0x10)])  # fmt: skip
    assert masks[0].any() and masks[1].any() and not masks.all(axis=1).any()
    mask_index = np.full(baselines, 255, u8)
    mask_index[:10], mask_index[10:30] = 1, 0
    seq.buffer("prepare:source").set(queue, source)
    seq.buffer("prepare:auto_source").set(queue, auto_source)
    seq.buffer("prepare:channel_flags").set(queue, masks)
    seq.buffer("prepare:mask_index").set(queue, mask_index)
    prepare_host = host.PrepareHost(scale, lost_flag, weight_scale)
    flagger_host = host.FlaggerHost(host.BackgroundMedianFilterHost(13), host.NoiseEstMADHost(),
                                    host.ThresholdSumHost(11.0))  # fmt: skip
    averager = host.AveragerHost(channels, baselines, cf, full)
    for d in range(3):
        baseline_flags = np.zeros(baselines, u8)
        baseline_flags[always] = off_target
        if d == 1:
            baseline_flags[once] = off_target
        vis_in = chain_dump(20 + d, channels, in_baselines)
        seq.buffer("prepare:vis_in").set(queue, vis_in)
        seq.buffer("prepare:baseline_flags").set(queue, baseline_flags)
        prepare()
        flagger()
        accumulate()
        vis, input_flags, weights = prepare_host(vis_in, source, masks, auto_source,
                                                 baseline_flags, mask_index)  # fmt: skip
        flags = flagger_host(vis, input_flags)
        averager.add(vis, flags, weights, input_flags=input_flags)
        for name, w in zip(("vis", "input_flags", "weights", "flags"),
                           (vis, input_flags, weights, flags)):  # fmt: skip
            assert_same(w, seq.buffer(name).get(queue), f"{name}, dump {d}")
        assert np.all(input_flags[:, always] & off_target)
        assert np.all((input_flags[:, once] & off_target != 0) == (d == 1))
        assert np.all((input_flags[:, :10] & 0x10 != 0) == (masks[1] != 0)[:, np.newaxis])
        assert not (input_flags[:, 10:] & 0x10).any() and not (input_flags[:, 30:] & 0x30).any()
    finalise()
    want = averager.finalise()
    got = [seq.buffer("finalise:" + name).get(queue) for name in ("vis", "weights", "flags")]
    for name, w, g in zip(("vis", "weights", "flags"), want, got):
        assert_same(w, g, name)
    # all contributions of the baseline that was off target throughout were flagged: its outputs
    # carry the bit; the one that was off target in one dump of three had data, and do not
    assert np.all(got[2][:, always] & off_target)
    assert not (got[2][:, once] & off_target).any()
