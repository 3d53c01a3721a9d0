"""A block of dumps added in one launch on the GPU (``rfi.ingest.AccumulateBlockTemplate``,
``ksp_average_accumulate_block``): every comparison is exact, against
``rfi.host.AveragerHost.add`` called dump by dump in dump order. uint8 values and float32 bit
patterns must be equal; a NaN is accepted only where the host has a NaN (its sign and payload
are not arithmetic). tests/test_accumulate_block.py shows, without a GPU, that the data used
here gives other bit patterns when the dumps are added in another order.

A lane owns a run of 16 baselines, and runs are dealt to 256-thread workgroups row after row:
a row ends in a partial run, which goes element by element, unless baselines is a multiple of
16; a wavefront spans 1024 baselines and a workgroup 4096.
"""

import ctypes

import numpy as np
import pytest

from tests import inputs
from tests import inputs_accumulate_block as data
from tests.subviews import SENTINEL, CompactViews, flat_device_array, poison_array, sentinel_array

pytestmark = pytest.mark.gpu

BASELINES = [1, 15, 16, 17, 63, 64, 65, 257, 1025, 4097]
CHANNELS = [1, 2, 7]
DUMPS = [1, 2, 3, 8]
MODES = ["NONE", "CHANNEL", "FULL"]
ACC = ("acc_vis", "acc_weights", "acc_flags")
OUT = ("vis", "weights", "flags")


@pytest.fixture(scope="module")
def context():
    from katsdpsigproc_amd import accel

    return accel.create_some_context(interactive=False)


@pytest.fixture(scope="module")
def command_queue(context):
    return context.create_command_queue()


def modes():
    from katsdpsigproc_amd.rfi import host

    return host.BackgroundFlags


def upload(queue, array, values, poison):
    """`values` into `array`; its padding gets what no result may depend on (`poison`: NaN or
    0xFF, for an input) or sentinel bytes (an accumulator)."""
    if poison:
        size = int(np.prod(array.padded_shape))
        raw = poison_array(size, array.dtype).reshape(array.padded_shape)
    else:
        raw = sentinel_array(array.padded_shape, array.dtype)
    raw[..., : array.shape[-1]] = values
    queue.enqueue_write_buffer(array.buffer, raw)


def read_checked(queue, array, name):
    """The data of `array`, after checking that its padding still holds the sentinel."""
    raw = np.empty(array.padded_shape, array.dtype)
    queue.enqueue_read_buffer(array.buffer, raw)
    padding = np.ascontiguousarray(raw[..., array.shape[-1] :]).view(np.uint8)
    assert np.all(padding == SENTINEL), f"wrote into the padding of {name}"
    return np.ascontiguousarray(raw[..., : array.shape[-1]])


class Block:
    """An AccumulateBlock operation with every row padded by at least `pad` more elements
    than its slots ask for: poison in the padding of the inputs, sentinels in that of the
    accumulators, which start at zero."""

    def __init__(self, context, queue, channels, baselines, dumps, use_weights=True, mode="NONE",
                 pad=0):  # fmt: skip
        from katsdpsigproc_amd import accel
        from katsdpsigproc_amd.rfi import ingest

        self.queue = queue
        self.use_weights, self.mode = use_weights, mode
        self.fn = ingest.AccumulateBlockTemplate(
            context, dumps, use_weights=use_weights, input_flags=modes()[mode]).instantiate(
            queue, channels, baselines)  # fmt: skip
        if pad:
            dims = {id(slot.dimensions[1]): slot.dimensions[1]
                    for slot in self.fn.slots.values() if len(slot.shape) == 2}  # fmt: skip
            for dim in dims.values():
                accel.Dimension(dim.size, min_padded_size=dim.size + pad).link(dim)
        for name in ACC:
            self.fn.ensure_bound(name)
            assert self.fn.buffer(name).padded_shape[1] >= baselines + pad
            upload(queue, self.fn.buffer(name), 0, poison=False)

    def load(self, selected):
        """The dumps of `selected` (inputs_accumulate_block.select) into the slots of the
        first dumps; `n_dumps` is set to their number."""
        fn = self.fn
        fn.n_dumps = len(selected)
        fn.ensure_all_bound()
        for d, (vis, flags, weights, mask) in enumerate(selected):
            upload(self.queue, fn.buffer(f"vis{d}"), vis, poison=True)
            upload(self.queue, fn.buffer(f"flags{d}"), flags, poison=True)
            if self.use_weights:
                upload(self.queue, fn.buffer(f"weights{d}"), weights, poison=True)
            if self.mode == "FULL":
                upload(self.queue, fn.buffer(f"input_flags{d}"), mask, poison=True)
        if self.mode == "CHANNEL":
            upload(self.queue, fn.buffer("input_flags"), selected[0][3], poison=True)

    def accumulators(self):
        return tuple(read_checked(self.queue, self.fn.buffer(name), name) for name in ACC)


def check_shape(context, queue, channels, baselines, dumps, use_weights=True, mode="NONE", pad=0,
                n_dumps=None):  # fmt: skip
    """A block from zero and the same block once more on top of it, each compared with the
    host. With `n_dumps` below `dumps` the slots of the later dumps are bound and hold NaN and
    0xFF, which must not be read."""
    n_dumps = dumps if n_dumps is None else n_dumps
    selected = data.select(data.make_dumps(channels, baselines)[:n_dumps], use_weights, mode)
    block = Block(context, queue, channels, baselines, dumps, use_weights, mode, pad)
    if n_dumps < dumps:
        block.fn.ensure_all_bound()
        for name, slot in block.fn.slots.items():
            if name not in ACC:
                array = slot.buffer
                queue.enqueue_write_buffer(
                    array.buffer, poison_array(int(np.prod(array.padded_shape)), array.dtype).reshape(
                        array.padded_shape))  # fmt: skip
    block.load(selected)
    assert block.fn.n_dumps == n_dumps
    want = None
    for round_ in range(2):
        block.fn()
        want = data.host_accumulate(selected, mode, start=want)
        for name, w, g in zip(ACC, want, block.accumulators()):
            data.assert_same(w, g, f"{name} {channels}x{baselines}, {n_dumps} of {dumps} dumps, "
                                   f"weights {use_weights}, {mode}, block {round_}")  # fmt: skip


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("use_weights", [True, False])
@pytest.mark.parametrize("dumps", DUMPS)
def test_shapes(dumps, use_weights, mode, context, command_queue):
    for channels in CHANNELS:
        for baselines in BASELINES:
            check_shape(context, command_queue, channels, baselines, dumps, use_weights, mode)


def test_tall(context, command_queue):
    """More rows than a grid dimension of 65535 could number."""
    check_shape(context, command_queue, 70000, 3, 2)


@pytest.mark.parametrize("use_weights, mode", [(True, "NONE"), (False, "CHANNEL"), (True, "FULL")])
@pytest.mark.parametrize("n_dumps", [1, 7])
def test_short_block(n_dumps, use_weights, mode, context, command_queue):
    """`n_dumps` of 1 and dumps - 1 on a template of 8: the rest is not read."""
    for channels, baselines in [(7, 65), (2, 1025), (3, 16), (1, 1)]:
        check_shape(context, command_queue, channels, baselines, 8, use_weights, mode,
                    n_dumps=n_dumps)  # fmt: skip


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("channels, baselines, pad", [(8, 65, 29), (7, 1025, 3), (8, 256, 16)])
def test_padding(channels, baselines, pad, mode, context, command_queue):
    """Rows padded beyond what the slots ask for; an odd pad is rounded up to the alignment
    (still the 16-byte path), and check_shape looks at the sentinels in every accumulator's
    padding."""
    check_shape(context, command_queue, channels, baselines, 3, True, mode, pad=pad)


def test_the_same_buffer_as_two_dumps(context, command_queue):
    """The inputs are read-only: dump 1 may be dump 0 again."""
    channels, baselines = 7, 65
    selected = data.select(data.make_dumps(channels, baselines)[:1], True, "FULL")
    block = Block(context, command_queue, channels, baselines, 2, True, "FULL")
    block.load(selected)
    fn = block.fn
    fn.bind(**{f"{kind}1": fn.buffer(f"{kind}0") for kind in ("vis", "flags", "weights", "input_flags")})
    fn.n_dumps = 2
    fn()
    for name, w, g in zip(ACC, data.host_accumulate(selected * 2, "FULL"), block.accumulators()):
        data.assert_same(w, g, name)


@pytest.mark.parametrize("mode", MODES)
def test_against_single_launches(mode, context, command_queue):
    """One block launch against as many launches of the existing Accumulate on the same
    inputs, device against device (and both against the host)."""
    from katsdpsigproc_amd.rfi import device

    queue = command_queue
    channels, baselines, dumps = 7, 1025, 8
    selected = data.select(data.make_dumps(channels, baselines), True, mode)
    block = Block(context, queue, channels, baselines, dumps, True, mode)
    block.load(selected)
    single = device.AccumulateTemplate(context, True, modes()[mode]).instantiate(
        queue, channels, baselines)  # fmt: skip
    single.ensure_all_bound()
    for name in ACC:
        single.buffer(name).zero(queue)
    for round_ in range(2):
        block.fn()
        for d in range(dumps):
            single.bind(vis=block.fn.buffer(f"vis{d}"), flags=block.fn.buffer(f"flags{d}"),
                        weights=block.fn.buffer(f"weights{d}"))  # fmt: skip
            if mode == "FULL":
                single.bind(input_flags=block.fn.buffer(f"input_flags{d}"))
            elif mode == "CHANNEL":
                single.bind(input_flags=block.fn.buffer("input_flags"))
            single()
    want = data.host_accumulate(selected * 2, mode)
    for name, w, g in zip(ACC, want, block.accumulators()):
        data.assert_same(w, g, f"{name}, block against host")
        data.assert_same(single.buffer(name).get(queue), g, f"{name}, block against launches")


def check_raw_abi(context, queue, mode, n_dumps, baselines, offset, strides, odd_one_out=None,
                  make_views=None):
    """The C function on sub-views `offset` elements into their allocations with the row
    stride `strides` gives each kind; `odd_one_out`, (dump, offset), moves the `vis` of that
    dump alone. The accumulators start from what two other dumps leave. `make_views` makes the
    arrays (tests/subviews.py: CompactViews unless given); the strides the launcher gets are
    those of the views it made."""
    from katsdpsigproc_amd import _lib

    make_views = make_views or CompactViews(context, queue)
    strides = dict(strides)

    def make(name, dtype, value, at=offset, poison=False):
        view = make_views(name, dtype, value, strides[name], at, poison)[0]
        strides[name] = view.stride
        return view

    channels = 6
    dumps = data.make_dumps(channels, baselines)
    selected = data.select(dumps[:n_dumps], True, mode)
    start = data.host_accumulate(data.select(dumps[6:8], True, mode, False), mode)
    dtypes = {"vis": np.complex64, "weights": np.float32, "flags": np.uint8}
    acc = {name: make(name, dtypes[name[4:]], value) for name, value in zip(ACC, start)}
    views = {"vis": [], "flags": [], "weights": [], "mask": []}
    for d, (vis, flags, weights, mask) in enumerate(selected):
        vis_offset = odd_one_out[1] if odd_one_out and odd_one_out[0] == d else offset
        views["vis"].append(make("vis", np.complex64, vis, vis_offset, poison=True))
        views["flags"].append(make("flags", np.uint8, flags, poison=True))
        views["weights"].append(make("weights", np.float32, weights, poison=True))
        if mode == "CHANNEL" and d == 0:
            views["mask"] = [flat_device_array(context, queue, np.uint8, mask[np.newaxis, :],
                                               channels, offset, poison=True)[0]] * n_dumps  # fmt: skip
        elif mode == "FULL":
            views["mask"].append(make("mask", np.uint8, mask, poison=True))

    def pointers(kind):
        return (ctypes.c_void_p * n_dumps)(*[view.address for view in views[kind]])

    _lib.call("ksp_average_accumulate_block", context.device.index, ctypes.c_void_p(queue.stream),
              n_dumps, pointers("vis"), pointers("flags"), pointers("weights"),
              pointers("mask") if mode != "NONE" else None, modes()[mode].value,
              acc["acc_vis"].ptr, acc["acc_weights"].ptr, acc["acc_flags"].ptr, channels,
              baselines, strides["vis"], strides["flags"], strides["weights"], strides["mask"],
              strides["acc_vis"], strides["acc_weights"], strides["acc_flags"])  # fmt: skip
    queue.finish()
    want = data.host_accumulate(selected, mode, start=start)
    for name, w in zip(ACC, want):
        data.assert_same(w, acc[name].read(name), f"{name}, {mode}, offset {offset}")
    for kind, members in views.items():
        for d, view in enumerate(members):
            view.read(f"{kind}{d}")  # an input: not one byte of its allocation has changed


ODD_STRIDES = {"vis": 41, "flags": 39, "weights": 43, "mask": 45, "acc_vis": 37,
               "acc_weights": 47, "acc_flags": 49}  # fmt: skip
# multiples of 16 elements: with a pointer that is 16-byte aligned every row start is
ALIGNED_STRIDES = {"vis": 48, "flags": 64, "weights": 80, "mask": 96, "acc_vis": 64,
                   "acc_weights": 48, "acc_flags": 112}  # fmt: skip


@pytest.mark.parametrize("offset", [1, 4, 12])
@pytest.mark.parametrize("mode", MODES)
def test_raw_abi_unaligned(mode, offset, context, command_queue):
    """Sub-views: pointers `offset` elements into their allocations, odd strides, a stride of
    its own per kind: the element path for every run."""
    check_raw_abi(context, command_queue, mode, 3, 37, offset, ODD_STRIDES)


@pytest.mark.parametrize("baselines", [1, 15, 16, 17, 33])
def test_raw_abi_unaligned_ragged(baselines, context, command_queue):
    """The same at the widths around a run of 16, a full block of 8."""
    check_raw_abi(context, command_queue, "FULL", 8, baselines, 1, ODD_STRIDES)


@pytest.mark.parametrize("mode", MODES)
def test_raw_abi_offset_aligned(mode, context, command_queue):
    """Offset 16 with strides that keep every row start a multiple of 16 bytes: sub-views on
    the 16-byte path (two whole runs and a ragged one per row)."""
    check_raw_abi(context, command_queue, mode, 3, 37, 16, ALIGNED_STRIDES)


@pytest.mark.parametrize("odd_one_out", [(0, 17), (1, 1), (2, 3)])
def test_raw_abi_one_misaligned_dump(odd_one_out, context, command_queue):
    """Everything aligned but the `vis` of one dump, which is 8 bytes off a multiple of 16:
    the whole call goes element by element."""
    check_raw_abi(context, command_queue, "FULL", 3, 37, 16, ALIGNED_STRIDES, odd_one_out)


def test_host_from_device(context, command_queue):
    from katsdpsigproc_amd.rfi import device, host, ingest

    channels, baselines, cf = 12, 70, 3
    selected = data.select(data.make_dumps(channels, baselines), True, "CHANNEL")
    on_device = ingest.BlockAveragerHostFromDevice(
        ingest.AccumulateBlockTemplate(context, 3, input_flags=modes().CHANNEL),
        device.FinaliseTemplate(context, channel_factor=cf), command_queue, channels, baselines)
    on_host = host.AveragerHost(channels, baselines, cf, modes().CHANNEL)
    for round_ in range(2):  # finalise clears both
        for block in (selected[:3], selected[3:5]):  # a full block and a short one
            vis, flags, weights, masks = (list(column) for column in zip(*block))
            if round_:
                weights[1] = None  # no weights means 1 everywhere
            on_device.add_block(vis, flags, weights, input_flags=masks)
            for v, f, w, m in zip(vis, flags, weights, masks):
                on_host.add(v, f, w, input_flags=m)
        for name, want, got in zip(OUT, on_host.finalise(), on_device.finalise()):
            data.assert_same(want, got, f"{name}, round {round_}")


def test_behind_the_flagger(context, command_queue):
    """Three output intervals of four dumps: the fused flagger, bound to one dump after the
    other, writes the flags the block then reads, and Finalise (clear=True) closes the
    interval; `vis`, `flags` and the channel mask are shared. Against FlaggerHost +
    AveragerHost."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import device, host, ingest

    queue = command_queue
    channels, baselines, cf, dumps = 64, 40, 4, 4
    channel = modes().CHANNEL
    flagger = device.FlaggerDeviceTemplate(
        device.BackgroundMedianFilterDeviceTemplate(context, 13, use_flags=channel),
        device.NoiseEstMADTDeviceTemplate(context, channels),
        device.ThresholdSumDeviceTemplate(context),
        fused=True, tuning={"vis_pad": 0},
    ).instantiate(queue, channels, baselines, threshold_args={"n_sigma": 11.0})
    assert isinstance(flagger, device.FusedFlaggerDevice)
    block = ingest.AccumulateBlockTemplate(context, dumps, use_weights=False,
                                           input_flags=channel).instantiate(
        queue, channels, baselines)  # fmt: skip
    finalise = device.FinaliseTemplate(context, channel_factor=cf, clear=True).instantiate(
        queue, channels, baselines)  # fmt: skip
    # the flagger serves every dump in turn: its padding is tied to the block's by the dimensions
    for name in ("vis", "flags"):
        block.slots[name + "0"].dimensions[1].link(flagger.slots[name].dimensions[1])
    block.slots["input_flags"].dimensions[0].link(flagger.slots["input_flags"].dimensions[0])
    seq = accel.OperationSequence(
        queue, [("block", block), ("finalise", finalise)],
        compounds={name: ["block:" + name, "finalise:" + name] for name in ACC})
    seq.ensure_all_bound()
    for name in ACC:
        seq.buffer(name).zero(queue)
    mask = inputs.channel_mask(channels, seed=4, fraction=1.0 / 8.0) * np.uint8(0x20)
    assert mask.any() and not mask.all()
    block.buffer("input_flags").set(queue, mask)
    flagger.bind(input_flags=block.buffer("input_flags"))
    flagger_host = host.FlaggerHost(host.BackgroundMedianFilterHost(13), host.NoiseEstMADHost(),
                                    host.ThresholdSumHost(11.0))  # fmt: skip
    averager = host.AveragerHost(channels, baselines, cf, channel)
    for interval in range(3):
        flagged = 0
        for d in range(dumps):
            seed = 100 * interval + d
            vis = inputs.add_rfi(inputs.generate_data(channels, baselines, seed=20 + seed),
                                 seed=30 + seed)  # fmt: skip
            block.buffer(f"vis{d}").set(queue, vis)
            flagger.bind(vis=block.buffer(f"vis{d}"), flags=block.buffer(f"flags{d}"))
            flagger()
            want_flags = flagger_host(vis, mask)
            np.testing.assert_array_equal(want_flags, block.buffer(f"flags{d}").get(queue))
            flagged += np.count_nonzero(want_flags)
            averager.add(vis, want_flags, input_flags=mask)
        assert flagged > 0
        block()
        finalise()
        want = averager.finalise()
        for name, w in zip(OUT, want):
            data.assert_same(w, seq.buffer("finalise:" + name).get(queue), f"{name}, interval {interval}")
        # spikes were left out: the averages are noise, not the 50 to 70 of the injected RFI
        assert np.abs(want[0]).max() < 10
