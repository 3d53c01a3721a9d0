"""Flag-aware averaging on the GPU (``rfi.device.AccumulateTemplate`` / ``FinaliseTemplate``,
``ksp_average_accumulate`` / ``ksp_average_finalise``): every comparison is exact, against
``rfi.host.AveragerHost``. uint8 values and float32 bit patterns must be equal; a NaN is
accepted only where the host has a NaN (its sign and payload are not arithmetic)."""

import ctypes

import numpy as np
import pytest

from tests import inputs
from tests.subviews import SENTINEL, CompactViews, flat_device_array, read_flat, sentinel_array

pytestmark = pytest.mark.gpu

# A lane owns a run of 16 baselines, and runs are dealt to 256-thread workgroups row after
# row: a row ends in a partial run unless baselines is a multiple of 16, a wavefront spans
# 1024 baselines and a workgroup 4096.
RUN = 16
WORKGROUP_COLS = 256 * RUN
BASELINES = [1, 3, 4, 5, 15, 16, 17, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025,
             WORKGROUP_COLS - 1, WORKGROUP_COLS, WORKGROUP_COLS + 1]  # fmt: skip
CHANNELS = [1, 2, 7, 8]
N_DUMPS = 4


@pytest.fixture(scope="module")
def context():
    from katsdpsigproc_amd import accel

    return accel.create_some_context(interactive=False)


@pytest.fixture(scope="module")
def command_queue(context):
    return context.create_command_queue()


def modes():
    from katsdpsigproc_amd.rfi import device

    return device.BackgroundFlags


def make_dumps(rs, channels, baselines, use_weights=True, mode="NONE"):
    """N_DUMPS of (vis, flags, weights or None, input_flags or None).

    Samples fall into classes by column (by position where there are fewer than 8 columns):
    never flagged, flagged in every dump (by every row: the outputs of any channel_factor are
    then all-flagged), flagged in the first dump only, flagged in the last dump only, and
    flagged at random in about half the dumps, with a different bit per dump. Weights are
    uniform in [0.5, 2] with some exact zeros; a few visibilities are around 2**-70 (their
    products with a flagged weight are denormal), a few are NaN or infinite."""
    shape = (channels, baselines)
    index = np.arange(baselines)[np.newaxis, :] + np.zeros(shape, int)
    if baselines < 8:
        index = np.arange(channels * baselines).reshape(shape)
    cls = index % 8
    dumps = []
    for d in range(N_DUMPS):
        vis = (rs.standard_normal(shape) + 1j * rs.standard_normal(shape)).astype(np.complex64)
        tiny = rs.random_sample(shape) < 0.05
        vis[tiny] *= np.float32(2.0**-70)
        special = rs.random_sample(shape)
        vis[special < 0.01] = np.nan
        vis[(special >= 0.01) & (special < 0.02)] = np.inf
        vis[(special >= 0.02) & (special < 0.03)] = complex(1.0, -np.inf)
        bits = np.uint8(1 << d) | rs.randint(0, 256, shape).astype(np.uint8) & np.uint8(0xF0)
        flagged = rs.random_sample(shape) < 0.5
        flagged[cls == 0] = False
        flagged[cls == 1] = True
        flagged[cls == 2] = d == 0
        flagged[cls == 3] = d == N_DUMPS - 1
        flags = np.where(flagged, bits, 0).astype(np.uint8)
        weights = None
        if use_weights:
            weights = rs.uniform(0.5, 2.0, shape).astype(np.float32)
            weights[rs.random_sample(shape) < 0.1] = 0
        mask = None
        if mode == "CHANNEL":
            mask = np.where(rs.random_sample(channels) < 0.3, 0x08, 0).astype(np.uint8)
        elif mode == "FULL":
            mask = np.where(rs.random_sample(shape) < 0.3, 0x08, 0).astype(np.uint8)
            mask[cls == 0] = 0
        dumps.append((vis, flags, weights, mask))
    return dumps


def host_accumulate(dumps, mode="NONE"):
    """(acc_vis, acc_weights, acc_flags) of the host class after `dumps`."""
    from katsdpsigproc_amd.rfi import host

    channels, baselines = dumps[0][0].shape
    averager = host.AveragerHost(channels, baselines, 1, modes()[mode])
    for vis, flags, weights, mask in dumps:
        averager.add(vis, flags, weights, mask)
    return averager.acc_vis, averager.acc_weights, averager.acc_flags


def host_finalise(acc, channel_factor):
    """What the host class makes of accumulators `acc` (which are left alone)."""
    from katsdpsigproc_amd.rfi import host

    averager = host.AveragerHost(*acc[0].shape, channel_factor)
    averager.acc_vis[...], averager.acc_weights[...], averager.acc_flags[...] = acc
    return averager.finalise()


def assert_same(want, got, what=""):
    """Equal bit patterns, except that a NaN may stand where the host has a NaN."""
    assert want.dtype == got.dtype and want.shape == got.shape, what
    if want.dtype == np.uint8:
        np.testing.assert_array_equal(want, got, err_msg=what)
        return
    want = np.ascontiguousarray(want).view(np.float32)
    got = np.ascontiguousarray(got).view(np.float32)
    same = want.view(np.uint32) == got.view(np.uint32)
    both_nan = np.isnan(want) & np.isnan(got)
    bad = ~(same | both_nan)
    assert not bad.any(), (
        f"{what}: {np.count_nonzero(bad)} of {bad.size} differ, first at "
        f"{np.argwhere(bad)[0]}: want {want[bad][0]!r}, got {got[bad][0]!r}")  # fmt: skip


def write_padded(queue, array, data):
    """`data` into `array`, sentinel bytes into its padding."""
    raw = sentinel_array(array.padded_shape, array.dtype)
    raw[..., : array.shape[-1]] = data
    queue.enqueue_write_buffer(array.buffer, raw)


def read_checked(queue, array, name):
    """The data of `array`, after checking that its padding still holds the sentinel."""
    raw = np.empty(array.padded_shape, array.dtype)
    queue.enqueue_read_buffer(array.buffer, raw)
    padding = np.ascontiguousarray(raw[..., array.shape[-1] :]).view(np.uint8)
    assert np.all(padding == SENTINEL), f"wrote into the padding of {name}"
    return np.ascontiguousarray(raw[..., : array.shape[-1]])


ACC = ("acc_vis", "acc_weights", "acc_flags")
OUT = ("vis", "weights", "flags")


class Pair:
    """Accumulate and Finalise operations (one per channel factor) on shared accumulators,
    every row padded by at least `pad` more elements, the padding full of sentinels."""

    def __init__(self, context, queue, channels, baselines, channel_factors=(1,), clear=False,
                 use_weights=True, mode="NONE", pad=0):  # fmt: skip
        from katsdpsigproc_amd import accel
        from katsdpsigproc_amd.rfi import device

        self.queue = queue
        self.accumulate = device.AccumulateTemplate(
            context, use_weights=use_weights, input_flags=modes()[mode]).instantiate(
            queue, channels, baselines)  # fmt: skip
        self.finalise = {
            cf: device.FinaliseTemplate(context, channel_factor=cf, clear=clear).instantiate(
                queue, channels, baselines) for cf in channel_factors}  # fmt: skip
        operations = [self.accumulate] + list(self.finalise.values())
        if pad:
            for op in operations:
                for slot in op.slots.values():
                    if len(slot.shape) == 2:
                        dim = slot.dimensions[1]
                        accel.Dimension(dim.size, min_padded_size=dim.size + pad).link(dim)
        names = ["accumulate"] + [f"finalise{cf}" for cf in channel_factors]
        self.sequence = accel.OperationSequence(
            queue, list(zip(names, operations)),
            compounds={acc: [f"{name}:{acc}" for name in names] for acc in ACC})  # fmt: skip
        self.sequence.ensure_all_bound()
        for name in ACC:
            buf = self.sequence.buffer(name)
            assert buf.padded_shape[1] >= baselines + pad
            write_padded(queue, buf, 0)
        for op in self.finalise.values():
            for name in OUT:
                assert op.buffer(name).padded_shape[1] >= baselines + pad
                write_padded(queue, op.buffer(name), sentinel_array((1,), op.buffer(name).dtype)[0])

    def add(self, vis, flags, weights=None, mask=None):
        fn = self.accumulate
        # poison in the padding of the inputs: flagged, NaN
        write_padded(self.queue, fn.buffer("vis"), vis)
        write_padded(self.queue, fn.buffer("flags"), flags)
        if weights is not None:
            write_padded(self.queue, fn.buffer("weights"), weights)
        if mask is not None:
            write_padded(self.queue, fn.buffer("input_flags"), mask)
        fn()

    def accumulators(self):
        return tuple(read_checked(self.queue, self.sequence.buffer(name), name) for name in ACC)

    def finish(self, channel_factor):
        op = self.finalise[channel_factor]
        op()
        return tuple(read_checked(self.queue, op.buffer(name), name) for name in OUT)


def factors(channels):
    return sorted({cf for cf in (1, 2, 7, channels) if channels % cf == 0})


def check_shape(context, queue, channels, baselines, seed, use_weights=True, mode="NONE", pad=0,
                channel_factors=None):  # fmt: skip
    """Accumulate N_DUMPS, compare the accumulators, then every channel factor from the same
    accumulators (clear=False, so this also shows that they are left unchanged)."""
    rs = np.random.RandomState(seed)
    dumps = make_dumps(rs, channels, baselines, use_weights, mode)
    channel_factors = channel_factors or factors(channels)
    pair = Pair(context, queue, channels, baselines, channel_factors, False, use_weights, mode, pad)
    for dump in dumps:
        pair.add(*dump)
    want_acc = host_accumulate(dumps, mode)
    got_acc = pair.accumulators()
    for name, want, got in zip(ACC, want_acc, got_acc):
        assert_same(want, got, f"{name} {channels}x{baselines}")
    for cf in channel_factors:
        want_out = host_finalise(want_acc, cf)
        got_out = pair.finish(cf)
        for name, want, got in zip(OUT, want_out, got_out):
            assert_same(want, got, f"{name} {channels}x{baselines} / {cf}")
        for name, before, after in zip(ACC, got_acc, pair.accumulators()):
            np.testing.assert_array_equal(before.view(np.uint8), after.view(np.uint8),
                                          err_msg=f"clear=False changed {name}")  # fmt: skip
    return want_out


@pytest.mark.parametrize("channels", CHANNELS)
def test_shapes(channels, context, command_queue):
    for baselines in BASELINES:
        check_shape(context, command_queue, channels, baselines, seed=channels * 10007 + baselines)


def test_data_covers_the_cases():
    """The generated dumps do contain what the tests are meant to exercise."""
    dumps = make_dumps(np.random.RandomState(1), 8, 65)
    acc = host_accumulate(dumps)
    vis, weights, flags = host_finalise(acc, 8)
    assert np.all(flags[:, 1::8] != 0) and not flags[:, 0::8].any()  # all-flagged / never flagged
    assert not flags[:, 2::8].any() and not flags[:, 3::8].any()  # absorbed, in both orders
    assert np.isnan(vis.real).any() and np.isfinite(vis.real).any()
    assert any((d[2] == 0).any() for d in dumps)
    products = np.abs((dumps[0][2] * np.float32(2.0**-64)) * dumps[0][0].real)
    assert ((products > 0) & (products < np.finfo(np.float32).tiny)).any()  # denormal products
    assert len({int(d[1][0, 1]) & 0x0F for d in dumps}) == N_DUMPS  # another bit per dump


def test_tall(context, command_queue):
    """More rows than a grid dimension of 65535 could number."""
    check_shape(context, command_queue, 70000, 3, seed=70000, channel_factors=(1, 7, 70000))


@pytest.mark.parametrize("mode", ["NONE", "CHANNEL", "FULL"])
@pytest.mark.parametrize("use_weights", [True, False])
def test_options(use_weights, mode, context, command_queue):
    for channels, baselines in [(7, 65), (8, 1025), (2, 16), (1, 1), (5, 15), (2, 17), (3, 33)]:
        check_shape(context, command_queue, channels, baselines, seed=baselines, mode=mode,
                    use_weights=use_weights)  # fmt: skip


@pytest.mark.parametrize("mode", ["NONE", "CHANNEL", "FULL"])
@pytest.mark.parametrize("channels, baselines, pad", [(8, 65, 29), (7, 1025, 3), (8, 256, 16)])
def test_padding(channels, baselines, pad, mode, context, command_queue):
    """Rows padded beyond what the slots ask for; an odd pad is rounded up to the alignment
    (still the 16-byte path), and check_shape looks at the sentinels in every padding."""
    check_shape(context, command_queue, channels, baselines, seed=pad, mode=mode, pad=pad)


@pytest.mark.parametrize("baselines", [1, 5, 15, 16, 17, 33, 257, 1040])
def test_clear(baselines, context, command_queue):
    channels = 8
    rs = np.random.RandomState(baselines)
    dumps = make_dumps(rs, channels, baselines)
    pair = Pair(context, command_queue, channels, baselines, (2,), clear=True, pad=5)
    for round_ in range(2):  # the second round starts from what the first one cleared
        for dump in dumps[2 * round_ : 2 * round_ + 2]:
            pair.add(*dump)
        want = host_finalise(host_accumulate(dumps[2 * round_ : 2 * round_ + 2]), 2)
        for name, w, g in zip(OUT, want, pair.finish(2)):
            assert_same(w, g, f"{name}, round {round_}")
        for name, acc in zip(ACC, pair.accumulators()):  # (checks their padding as well)
            assert not acc.view(np.uint8).any(), f"{name} was not cleared"


@pytest.mark.parametrize("offset", [1, 4, 12])
@pytest.mark.parametrize("mode", ["NONE", "CHANNEL", "FULL"])
def test_raw_abi_unaligned(mode, offset, context, command_queue):
    """Sub-views: pointers `offset` elements into their allocations, odd strides, a stride of
    its own per array."""
    check_raw_abi(mode, offset, 37, context, command_queue)


@pytest.mark.parametrize("baselines", [1, 15, 16, 17, 33])
@pytest.mark.parametrize("mode", ["NONE", "CHANNEL", "FULL"])
def test_raw_abi_unaligned_ragged(mode, baselines, context, command_queue):
    """The same one element into the allocations (4 bytes for the weights, 1 for the flags),
    at the widths around a run of 16: no run, a run short of one baseline, a whole run, runs
    followed by one baseline."""
    check_raw_abi(mode, 1, baselines, context, command_queue)


def check_raw_abi(mode, offset, baselines, context, command_queue, views=None):
    """`views` makes the arrays (tests/subviews.py: CompactViews unless given); the strides the
    launchers get are those of the views it made."""
    from katsdpsigproc_amd import _lib

    queue = command_queue
    views = views or CompactViews(context, queue)
    channels, cf = 6, 3
    dumps = make_dumps(np.random.RandomState(offset), channels, baselines, True, mode)
    strides = {"vis": 41, "flags": 39, "weights": 43, "mask": 45, "acc_vis": 37,
               "acc_weights": 47, "acc_flags": 49, "out_vis": 51, "out_weights": 37,
               "out_flags": 53}  # fmt: skip
    dtypes = {"vis": np.complex64, "weights": np.float32, "flags": np.uint8}

    def make(name, dtype, data, poison=False):
        made = views(name, dtype, data, strides[name], offset, poison)
        strides[name] = made[0].stride
        return made

    acc = {}
    for name in ACC:
        acc[name] = make(name, dtypes[name[4:]], np.zeros((channels, baselines), dtypes[name[4:]]))
    device_index = context.device.index
    stream = ctypes.c_void_p(queue.stream)
    for vis, flags, weights, mask in dumps:
        with views.scope():
            d_vis = make("vis", np.complex64, vis, poison=True)
            d_flags = make("flags", np.uint8, flags, poison=True)
            d_weights = make("weights", np.float32, weights, poison=True)
            if mode == "CHANNEL":
                d_mask = flat_device_array(context, queue, np.uint8, mask[np.newaxis, :], channels, offset, poison=True)
            elif mode == "FULL":
                d_mask = make("mask", np.uint8, mask, poison=True)
            else:
                d_mask = (None, None)
            _lib.call("ksp_average_accumulate", device_index, stream, d_vis[1], d_flags[1],
                      d_weights[1], d_mask[1], modes()[mode].value, acc["acc_vis"][1],
                      acc["acc_weights"][1], acc["acc_flags"][1], channels, baselines, strides["vis"],
                      strides["flags"], strides["weights"], strides["mask"], strides["acc_vis"],
                      strides["acc_weights"], strides["acc_flags"])  # fmt: skip
            queue.finish()  # the inputs of this dump go out of scope
            for name, view in (("vis", d_vis), ("flags", d_flags), ("weights", d_weights), ("mask", d_mask)):
                if view[0] is not None:
                    view[0].read(name)  # (asserts that nothing wrote to it)
    want_acc = host_accumulate(dumps, mode)
    for name, want in zip(ACC, want_acc):
        got = read_flat(queue, acc[name][0], (channels, baselines), strides[name], offset)
        assert_same(want, got, name)
    out = {}
    for name in OUT:
        dtype = dtypes[name]
        out[name] = make("out_" + name, dtype, sentinel_array((channels // cf, baselines), dtype))
    for clear in (0, 1):
        _lib.call("ksp_average_finalise", device_index, stream, acc["acc_vis"][1],
                  acc["acc_weights"][1], acc["acc_flags"][1], out["vis"][1], out["weights"][1],
                  out["flags"][1], channels, baselines, cf, clear, strides["acc_vis"],
                  strides["acc_weights"], strides["acc_flags"], strides["out_vis"],
                  strides["out_weights"], strides["out_flags"])  # fmt: skip
        for name, want in zip(OUT, host_finalise(want_acc, cf)):
            got = read_flat(queue, out[name][0], (channels // cf, baselines),
                            strides["out_" + name], offset)  # fmt: skip
            assert_same(want, got, f"{name}, clear={clear}")
        for name, want in zip(ACC, want_acc):
            got = read_flat(queue, acc[name][0], (channels, baselines), strides[name], offset)
            if clear:
                assert not got.view(np.uint8).any(), f"{name} was not cleared"
            else:
                assert_same(want, got, f"{name} after clear=0")


def test_host_from_device(context, command_queue):
    from katsdpsigproc_amd.rfi import device, host

    channels, baselines, cf = 12, 70, 3
    dumps = make_dumps(np.random.RandomState(11), channels, baselines, True, "CHANNEL")
    on_device = device.AveragerHostFromDevice(
        device.AccumulateTemplate(context, input_flags=modes().CHANNEL),
        device.FinaliseTemplate(context, channel_factor=cf), command_queue, channels, baselines)
    on_host = host.AveragerHost(channels, baselines, cf, modes().CHANNEL)
    for round_ in range(2):  # finalise clears both
        for vis, flags, weights, mask in dumps[2 * round_ : 2 * round_ + 2]:
            weights = None if round_ else weights  # no weights means 1 everywhere
            on_device.add(vis, flags, weights, input_flags=mask)
            on_host.add(vis, flags, weights, input_flags=mask)
        for name, want, got in zip(OUT, on_host.finalise(), on_device.finalise()):
            assert_same(want, got, f"{name}, round {round_}")


def test_behind_the_flagger(context, command_queue):
    """Three dumps through flagger -> accumulate -> finalise in one sequence, `vis`, `flags`
    and the channel mask shared, against FlaggerHost + AveragerHost."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import device, host

    queue = command_queue
    channels, baselines, cf = 64, 40, 4
    channel = modes().CHANNEL
    flagger = device.FlaggerDeviceTemplate(
        device.BackgroundMedianFilterDeviceTemplate(context, 13, use_flags=channel),
        device.NoiseEstMADTDeviceTemplate(context, channels),
        device.ThresholdSumDeviceTemplate(context),
        fused=True, tuning={"vis_pad": 0},
    ).instantiate(queue, channels, baselines, threshold_args={"n_sigma": 11.0})
    assert isinstance(flagger, device.FusedFlaggerDevice)
    accumulate = device.AccumulateTemplate(context, use_weights=False, input_flags=channel).instantiate(
        queue, channels, baselines)  # fmt: skip
    finalise = device.FinaliseTemplate(context, channel_factor=cf).instantiate(
        queue, channels, baselines)  # fmt: skip
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
    for name in device.FusedFlaggerDevice._OPTIONAL:
        del seq.slots["flagger:" + name]
    seq.ensure_all_bound()
    for name in ACC:
        seq.buffer(name).zero(queue)
    mask = inputs.channel_mask(channels, seed=4, fraction=1.0 / 8.0) * np.uint8(0x20)
    assert mask.any() and not mask.all()
    seq.buffer("input_flags").set(queue, mask)
    flagger_host = host.FlaggerHost(host.BackgroundMedianFilterHost(13), host.NoiseEstMADHost(),
                                    host.ThresholdSumHost(11.0))  # fmt: skip
    averager = host.AveragerHost(channels, baselines, cf, channel)
    flagged = 0
    for d in range(3):
        vis = inputs.add_rfi(inputs.generate_data(channels, baselines, seed=20 + d), seed=30 + d)
        seq.buffer("vis").set(queue, vis)
        flagger()
        accumulate()
        want_flags = flagger_host(vis, mask)
        np.testing.assert_array_equal(want_flags, seq.buffer("flags").get(queue))
        flagged += np.count_nonzero(want_flags)
        averager.add(vis, want_flags, input_flags=mask)
    assert flagged > 0
    finalise()
    want = averager.finalise()
    for name, w in zip(OUT, want):
        assert_same(w, seq.buffer("finalise:" + name).get(queue), name)
    # spikes were left out: the averages are noise, not the 50 to 70 of the injected RFI
    assert np.abs(want[0]).max() < 10
    # and once more through the sequence as a whole: one call per dump plus the final pass
    vis = inputs.add_rfi(inputs.generate_data(channels, baselines, seed=40), seed=41)
    seq.buffer("vis").set(queue, vis)
    seq()
    averager.add(vis, flagger_host(vis, mask), input_flags=mask)
    for name, w in zip(OUT, averager.finalise()):
        assert_same(w, seq.buffer("finalise:" + name).get(queue), name)
