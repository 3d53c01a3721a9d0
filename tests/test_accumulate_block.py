"""``rfi.ingest.AccumulateBlock`` without a GPU: argument errors, slot wiring and every launch
argument on the fake backend, the sequence between two ``Prepare`` and ``Finalise`` with the
fused flagger bound to one dump after the other, the host adapter's errors, the argument checks
of ``ksp_average_accumulate_block`` (which come before any device call), and that the data of
the GPU tests does tell one order of the dumps from another."""

import ctypes

import numpy as np
import pytest

from katsdpsigproc_amd import accel
from katsdpsigproc_amd.rfi import device, host, ingest
from tests import inputs_accumulate_block as data
from tests.fakes import FakeContext

NONE, CHANNEL, FULL = (host.BackgroundFlags.NONE, host.BackgroundFlags.CHANNEL,
                       host.BackgroundFlags.FULL)  # fmt: skip


@pytest.fixture
def context():
    return FakeContext()


@pytest.fixture
def queue(context):
    return context.create_command_queue()


def test_template_errors(context, queue):
    assert ingest.MAX_DUMPS == 8
    for dumps in (0, 9, -1):
        with pytest.raises(ValueError):
            ingest.AccumulateBlockTemplate(context, dumps)
    with pytest.raises(ValueError):
        ingest.AccumulateBlockTemplate(context, 2, input_flags=5)
    with pytest.raises(ValueError):
        ingest.AccumulateBlockTemplate(context, 2, tuning={"wgs": 256})
    template = ingest.AccumulateBlockTemplate(context, 3, tuning={})
    assert template.tuning == {} and template.dumps == 3
    assert ingest.AccumulateBlockTemplate.autotune(context, 3) == {}
    assert ingest.AccumulateBlockTemplate.host_class is host.AveragerHost
    assert ingest.AccumulateBlockTemplate.KERNEL == "ksp_average_accumulate_block"
    assert template.kernel.name == "ksp_average_accumulate_block"
    for channels, baselines in [(0, 4), (4, 0), (-4, 4)]:
        with pytest.raises(ValueError):
            template.instantiate(queue, channels, baselines)
    fn = template.instantiate(queue, 4, 4)
    assert isinstance(fn, ingest.AccumulateBlock) and fn.n_dumps == 3
    for n_dumps in (0, 4, -1):
        with pytest.raises(ValueError):
            fn.n_dumps = n_dumps
    assert fn.n_dumps == 3
    fn.n_dumps = 1
    assert fn.n_dumps == 1


def stride(fn, name):
    return fn.buffer(name).padded_shape[1]


@pytest.mark.parametrize("mode", [NONE, CHANNEL, FULL])
@pytest.mark.parametrize("use_weights", [True, False])
def test_wiring(use_weights, mode, context, queue):
    dumps = 3
    template = ingest.AccumulateBlockTemplate(context, dumps, use_weights=use_weights,
                                              input_flags=mode)  # fmt: skip
    fn = template.instantiate(queue, 300, 200)
    kinds = {"vis": np.complex64, "flags": np.uint8}
    if use_weights:
        kinds["weights"] = np.float32
    if mode == FULL:
        kinds["input_flags"] = np.uint8
    names = [f"{kind}{d}" for kind in kinds for d in range(dumps)]
    names += ["input_flags"] if mode == CHANNEL else []
    names += ["acc_vis", "acc_weights", "acc_flags"]
    assert list(fn.slots) == names
    for kind, dtype in kinds.items():
        for d in range(dumps):
            slot = fn.slots[f"{kind}{d}"]
            assert slot.shape == (300, 200) and slot.dtype == dtype
        # one dimension object per kind for the baselines, an own one per slot for the channels
        assert len({id(fn.slots[f"{kind}{d}"].dimensions[1]) for d in range(dumps)}) == 1
        assert len({id(fn.slots[f"{kind}{d}"].dimensions[0]) for d in range(dumps)}) == dumps
    if mode == CHANNEL:
        assert fn.slots["input_flags"].shape == (300,) and fn.slots["input_flags"].dtype == np.uint8
    for name, dtype in (("acc_vis", np.complex64), ("acc_weights", np.float32),
                        ("acc_flags", np.uint8)):  # fmt: skip
        assert fn.slots[name].shape == (300, 200) and fn.slots[name].dtype == dtype
    shared = [fn.slots[f"{kind}0"].dimensions[1] for kind in kinds]
    shared += [fn.slots[name].dimensions[1] for name in ("acc_vis", "acc_weights", "acc_flags")]
    assert len({id(dim) for dim in shared}) == len(shared)
    # padding asked of one dump's slot is every dump's of that kind, and nobody else's
    accel.Dimension(200, min_padded_size=500).link(fn.slots["flags1"].dimensions[1])
    accel.Dimension(200, min_padded_size=300).link(fn.slots["acc_weights"].dimensions[1])
    fn()
    assert [name for name, _ in queue.launches] == ["ksp_average_accumulate_block"]
    args = queue.launches[0][1]
    assert len(args) == 18
    assert int(args[0]) == dumps

    def pointers(kind):
        return [fn.buffer(f"{kind}{d}").buffer.ptr for d in range(dumps)]

    for arg in args[1:3]:
        assert isinstance(arg, ctypes.Array) and arg._type_ is ctypes.c_void_p and len(arg) == dumps
    assert list(args[1]) == pointers("vis") and list(args[2]) == pointers("flags")
    assert len(set(args[1])) == len(set(args[2])) == dumps
    if use_weights:
        assert isinstance(args[3], ctypes.Array) and list(args[3]) == pointers("weights")
    else:
        assert args[3] is None
    if mode == FULL:
        assert isinstance(args[4], ctypes.Array) and list(args[4]) == pointers("input_flags")
    elif mode == CHANNEL:
        assert isinstance(args[4], ctypes.Array)
        assert list(args[4]) == [fn.buffer("input_flags").buffer.ptr] * dumps
    else:
        assert args[4] is None
    assert int(args[5]) == mode.value
    assert args[6] is fn.buffer("acc_vis").buffer
    assert args[7] is fn.buffer("acc_weights").buffer
    assert args[8] is fn.buffer("acc_flags").buffer
    assert [int(a) for a in args[9:11]] == [300, 200]
    assert [int(a) for a in args[11:]] == [
        stride(fn, "vis0"), stride(fn, "flags0"), stride(fn, "weights0") if use_weights else 0,
        stride(fn, "input_flags0") if mode == FULL else 0, stride(fn, "acc_vis"),
        stride(fn, "acc_weights"), stride(fn, "acc_flags")]  # fmt: skip
    # rows of whole 128 bytes, except where more was asked for
    assert [stride(fn, f"vis{d}") for d in range(dumps)] == [208] * dumps
    assert [stride(fn, f"flags{d}") for d in range(dumps)] == [512] * dumps
    assert stride(fn, "acc_vis") == 208 and stride(fn, "acc_flags") == 256
    assert stride(fn, "acc_weights") == 320
    assert fn.parameters() == {"dumps": dumps, "use_weights": use_weights,
                               "input_flags": mode.name, "channels": 300, "baselines": 200}  # fmt: skip


@pytest.mark.parametrize("mode", [NONE, CHANNEL, FULL])
def test_short_block_leaves_later_dumps_unbound(mode, context, queue):
    dumps, n_dumps = 8, 3
    fn = ingest.AccumulateBlockTemplate(context, dumps, input_flags=mode).instantiate(queue, 12, 40)
    fn.n_dumps = n_dumps
    fn()
    kinds = ["vis", "flags", "weights"] + (["input_flags"] if mode == FULL else [])
    for kind in kinds:
        for d in range(dumps):
            assert fn.slots[f"{kind}{d}"].is_bound() == (d < n_dumps), (kind, d)
    args = queue.launches[0][1]
    assert int(args[0]) == n_dumps
    for arg, kind in zip(args[1:4], kinds):
        assert list(arg) == [fn.buffer(f"{kind}{d}").buffer.ptr for d in range(n_dumps)]
    if mode == FULL:
        assert list(args[4]) == [fn.buffer(f"input_flags{d}").buffer.ptr for d in range(n_dumps)]
    elif mode == CHANNEL:
        assert list(args[4]) == [fn.buffer("input_flags").buffer.ptr] * n_dumps
    # back to the full block: the rest is allocated on the way
    fn.n_dumps = dumps
    fn()
    assert all(slot.is_bound() for slot in fn.slots.values())
    assert int(queue.launches[1][1][0]) == dumps and len(queue.launches[1][1][1]) == dumps


def test_between_prepare_and_finalise(context, queue):
    """prepare x 2 -> fused flagger (FULL), bound to one dump after the other -> block of 2
    (weights, FULL) -> finalise: `vis`, `input_flags`, `weights` and the accumulators are each
    one buffer per dump, and the two dumps of a kind have one padded size."""
    channels, baselines, in_baselines = 4096, 200, 260
    prepares = [ingest.PrepareTemplate(context, weights=True, channel_flags=True).instantiate(
        queue, channels, baselines, in_baselines) for _ in range(2)]  # fmt: skip
    flagger = device.FlaggerDeviceTemplate(
        device.BackgroundMedianFilterDeviceTemplate(context, 13, use_flags=FULL),
        device.NoiseEstMADTDeviceTemplate(context, channels),
        device.ThresholdSumDeviceTemplate(context),
        tuning={"vis_pad": 0},
    ).instantiate(queue, channels, baselines, threshold_args={"n_sigma": 11.0})
    assert isinstance(flagger, device.FusedFlaggerDevice)
    block = ingest.AccumulateBlockTemplate(context, 2, input_flags=FULL).instantiate(
        queue, channels, baselines)  # fmt: skip
    finalise = device.FinaliseTemplate(context, channel_factor=8).instantiate(
        queue, channels, baselines)  # fmt: skip
    # The flagger serves both dumps, so it cannot be a member of either dump's compound: its
    # row padding is tied to the block's by linking the dimensions.
    for name in ("vis", "input_flags", "flags"):
        block.slots[name + "0"].dimensions[1].link(flagger.slots[name].dimensions[1])
    # more row padding than any of them asks for, asked of one member of one dump's compound
    accel.Dimension(baselines, min_padded_size=300).link(flagger.slots["vis"].dimensions[1])
    accel.Dimension(baselines, min_padded_size=400).link(prepares[1].slots["input_flags"].dimensions[1])
    accel.Dimension(baselines, min_padded_size=500).link(prepares[0].slots["weights"].dimensions[1])
    compounds = {name: ["block:" + name, "finalise:" + name]
                 for name in ("acc_vis", "acc_weights", "acc_flags")}  # fmt: skip
    for d in range(2):
        for name in ("vis", "input_flags", "weights"):
            compounds[f"{name}{d}"] = [f"prepare{d}:{name}", f"block:{name}{d}"]
    seq = accel.OperationSequence(
        queue, [("prepare0", prepares[0]), ("prepare1", prepares[1]), ("block", block),
                ("finalise", finalise)], compounds=compounds)  # fmt: skip
    for name in ("prepare0:vis", "block:vis1", "prepare1:weights", "block:acc_flags"):
        assert name not in seq.slots
    seq.ensure_all_bound()
    for d in range(2):
        prepares[d]()
        flagger.bind(vis=seq.buffer(f"vis{d}"), input_flags=seq.buffer(f"input_flags{d}"),
                     flags=seq.buffer(f"block:flags{d}"))  # fmt: skip
        flagger()
    block()
    finalise()
    assert [name for name, _ in queue.launches] == [
        "ksp_prepare", "ksp_flagger_fused", "ksp_prepare", "ksp_flagger_fused",
        "ksp_average_accumulate_block", "ksp_average_finalise"]  # fmt: skip
    launches = [launch[1] for launch in queue.launches]
    prep_args, flag_args, add_args, fin_args = launches[0:3:2], launches[1:4:2], launches[4], launches[5]
    for d in range(2):
        for name in ("vis", "input_flags", "weights"):
            assert prepares[d].buffer(name) is block.buffer(f"{name}{d}") is seq.buffer(f"{name}{d}")
        assert prep_args[d][4] is flag_args[d][0] is seq.buffer(f"vis{d}").buffer
        assert prep_args[d][5] is flag_args[d][1] is seq.buffer(f"input_flags{d}").buffer
        assert flag_args[d][2] is seq.buffer(f"block:flags{d}").buffer
        assert prep_args[d][6] is seq.buffer(f"weights{d}").buffer
    assert int(add_args[0]) == 2
    for arg, name in zip(add_args[1:5], ("vis", "block:flags", "weights", "input_flags")):
        assert list(arg) == [seq.buffer(f"{name}{d}").buffer.ptr for d in range(2)]
        assert arg[0] != arg[1]
    assert int(add_args[5]) == FULL.value
    strides = {name: [seq.buffer(f"{name}{d}").padded_shape[1] for d in range(2)]
               for name in ("vis", "input_flags", "weights", "block:flags")}  # fmt: skip
    # 300, 400 and 500 rounded up to whole 128-byte rows, whichever dump's slot was asked
    assert strides == {"vis": [304] * 2, "input_flags": [512] * 2, "weights": [512] * 2,
                       "block:flags": [256] * 2}  # fmt: skip
    assert [int(a) for a in add_args[11:15]] == [304, 256, 512, 512]
    for d in range(2):
        assert int(prep_args[d][11]) == int(flag_args[d][7]) == 304
        assert int(prep_args[d][12]) == int(flag_args[d][8]) == 512
        assert int(flag_args[d][9]) == 256 and int(prep_args[d][13]) == 512
    # the accumulators go from the block to the finishing pass
    assert add_args[6] is fin_args[0] and add_args[7] is fin_args[1] and add_args[8] is fin_args[2]
    assert seq.buffer("finalise:vis").shape == (channels // 8, baselines)


def test_host_from_device_errors(context, queue):
    vis = [np.zeros((4, 3), np.complex64)] * 2
    flags = [np.zeros((4, 3), np.uint8)] * 2
    weights = [np.ones((4, 3), np.float32)] * 2
    finalise = device.FinaliseTemplate(context)

    def adapter(dumps=2, **kwargs):
        return ingest.BlockAveragerHostFromDevice(
            ingest.AccumulateBlockTemplate(context, dumps, **kwargs), finalise, queue, 4, 3)

    plain = adapter()
    with pytest.raises(TypeError):
        plain.add_block(vis, flags, input_flags=[np.zeros(4, np.uint8)] * 2)
    for mode in (CHANNEL, FULL):
        with pytest.raises(TypeError):
            adapter(input_flags=mode).add_block(vis, flags)
    with pytest.raises(TypeError):
        adapter(use_weights=False).add_block(vis, flags, weights)
    for n in (0, 3):
        with pytest.raises(ValueError):
            plain.add_block(vis[:1] * n, flags[:1] * n)
    with pytest.raises(ValueError):
        plain.add_block(vis, flags[:1])
    with pytest.raises(ValueError):
        plain.add_block(vis, flags, weights[:1])
    with pytest.raises(ValueError):
        adapter(input_flags=FULL).add_block(vis, flags, input_flags=flags[:1])
    with pytest.raises(ValueError):  # one mask per block
        adapter(input_flags=CHANNEL).add_block(
            vis, flags, input_flags=[np.zeros(4, np.uint8), np.ones(4, np.uint8)])
    with pytest.raises(ValueError):
        ingest.BlockAveragerHostFromDevice(ingest.AccumulateBlockTemplate(context, 2),
                                           device.FinaliseTemplate(context, 3), queue, 4, 3)  # fmt: skip
    assert queue.launches == []
    # one set of accumulators, shared by the two operations; kernels in call order; a short
    # block, an entry without weights
    plain.add_block(vis, flags, [None, weights[1]])
    plain.add_block(vis[:1], flags[:1])
    plain.finalise()
    assert [name for name, _ in queue.launches] == [
        "ksp_average_accumulate_block", "ksp_average_accumulate_block", "ksp_average_finalise"]  # fmt: skip
    first, second, fin_args = (launch[1] for launch in queue.launches)
    assert (int(first[0]), len(first[1])) == (2, 2) and (int(second[0]), len(second[1])) == (1, 1)
    assert first[6] is fin_args[0] and first[7] is fin_args[1] and first[8] is fin_args[2]
    masked = adapter(input_flags=CHANNEL)
    masked.add_block(vis, flags, input_flags=[np.ones(4, np.uint8)] * 2)
    assert int(queue.launches[-1][1][5]) == CHANNEL.value


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

    def ptrs(*values):
        return (ctypes.c_void_p * len(values))(*values)

    ok = ptrs(64, 64, 64)
    hole = ptrs(64, None, 64)  # the NULL entry is within n_dumps
    behind = ptrs(64, 64, None)  # ... and here it is not

    def call(n_dumps=2, vis=ok, flags=ok, weights=ok, input_flags=None, mode=0, acc_vis=p,
             acc_weights=p, acc_flags=p, channels=4, baselines=8, vis_stride=8, flags_stride=8,
             weights_stride=8, input_flags_stride=8, acc_vis_stride=8, acc_weights_stride=8,
             acc_flags_stride=8):  # fmt: skip
        rc = lib.ksp_average_accumulate_block(
            0, None, n_dumps, vis, flags, weights, input_flags, mode, acc_vis, acc_weights,
            acc_flags, channels, baselines, vis_stride, flags_stride, weights_stride,
            input_flags_stride, acc_vis_stride, acc_weights_stride, acc_flags_stride)  # fmt: skip
        assert rc != 0
        return _lib.last_error()

    for n_dumps in (0, 9, -1):
        assert "n_dumps must be 1..8" in call(n_dumps=n_dumps, vis=ptrs(*[64] * 9))
    assert "invalid argument: vis is NULL" in call(vis=None)
    assert "invalid argument: flags is NULL" in call(flags=None)
    assert "invalid argument: acc_vis is NULL" in call(acc_vis=None)
    assert "invalid argument: acc_weights is NULL" in call(acc_weights=None)
    assert "invalid argument: acc_flags is NULL" in call(acc_flags=None)
    assert "input_flags is NULL" in call(mode=1)
    assert "input_flags is NULL" in call(mode=2)
    assert "input_flags given" in call(input_flags=ok)
    assert "input_flags_mode" in call(mode=3, input_flags=ok)
    assert "input_flags_mode" in call(mode=-1, input_flags=ok)
    assert "an entry of vis is NULL" in call(vis=hole)
    assert "an entry of flags is NULL" in call(flags=hole)
    assert "an entry of weights is NULL" in call(weights=hole)
    assert "an entry of input_flags is NULL" in call(mode=1, input_flags=hole)
    assert "an entry of input_flags is NULL" in call(mode=2, input_flags=hole)
    assert "an entry of vis is NULL" in call(n_dumps=3, vis=behind)
    # an entry behind n_dumps is not looked at: the call gets as far as the next check
    assert "channels" in call(vis=behind, flags=behind, weights=behind, channels=0)
    assert "channels" in call(channels=0)
    assert "baselines" in call(baselines=0)
    small = "_stride is smaller than baselines"
    assert "invalid argument: vis" + small in call(vis_stride=7)
    assert "acc_vis" not in _lib.last_error()
    assert "invalid argument: flags" + small in call(flags_stride=7)
    assert "invalid argument: weights" + small in call(weights_stride=7)
    assert "channels" in call(weights=None, weights_stride=7, channels=0)  # (ignored without weights)
    assert "invalid argument: input_flags" + small in call(
        mode=2, input_flags=ok, input_flags_stride=7)  # fmt: skip
    assert "channels" in call(mode=1, input_flags=ok, input_flags_stride=7, channels=0)
    assert "invalid argument: acc_vis" + small in call(acc_vis_stride=7)
    assert "invalid argument: acc_weights" + small in call(acc_weights_stride=7)
    assert "invalid argument: acc_flags" + small in call(acc_flags_stride=7)
    # the order of the checks: everything wrong at once, then only every stride
    strides = {name + "_stride": -1 for name in (
        "vis", "flags", "weights", "input_flags", "acc_vis", "acc_weights", "acc_flags")}  # fmt: skip
    assert "invalid argument: vis is NULL" in call(
        vis=None, flags=None, weights=None, acc_vis=None, acc_weights=None, acc_flags=None,
        channels=0, baselines=0, **strides)  # fmt: skip
    assert "invalid argument: vis" + small in call(mode=2, input_flags=ok, **strides)
    # 2**31 workgroups of 256 runs of 16 baselines and one more
    assert "too large" in call(channels=2**31 - 1, baselines=2**31 - 1, vis_stride=2**31 - 1,
                               flags_stride=2**31 - 1, weights_stride=2**31 - 1,
                               acc_vis_stride=2**31 - 1, acc_weights_stride=2**31 - 1,
                               acc_flags_stride=2**31 - 1)  # fmt: skip


@pytest.mark.parametrize("mode", ["NONE", "CHANNEL", "FULL"])
@pytest.mark.parametrize("use_weights", [True, False])
def test_the_data_tells_the_order_of_the_dumps(use_weights, mode):
    """The GPU tests compare with ``AveragerHost.add`` called in dump order. That shows the
    kernel's order only if another order gives another result: for the data they use, and
    every block longer than one dump, the dumps added in reverse differ in the bit patterns of
    the accumulated visibilities (and, from three dumps on, of the accumulated weights, where
    there are weights)."""
    dumps = data.make_dumps(7, 65)
    first = data.host_accumulate(data.select(dumps[:2], use_weights, mode), mode)
    for n_dumps in (2, 3, 7, 8):
        block = data.select(dumps[:n_dumps], use_weights, mode)
        forward = data.host_accumulate(block, mode, start=first)
        backward = data.host_accumulate(block[::-1], mode, start=first)
        differ = ~data.same_bits(forward[0], backward[0])
        assert differ.any(), f"{n_dumps} dumps in reverse accumulate the same visibilities"
        assert np.count_nonzero(differ) > differ.size // 100
        np.testing.assert_array_equal(forward[2], backward[2])  # an OR has no order
    # from zero, too, once there are three terms
    block = data.select(dumps[:3], use_weights, mode)
    forward, backward = data.host_accumulate(block, mode), data.host_accumulate(block[::-1], mode)
    assert not data.same_bits(forward[0], backward[0]).all()
    if use_weights:
        assert not data.same_bits(forward[1], backward[1]).all()


def test_the_data_covers_the_cases():
    """The generated dumps do contain what the tests are meant to exercise."""
    dumps = data.make_dumps(8, 65)
    block = data.select(dumps)
    acc_vis, acc_weights, acc_flags = data.host_accumulate(block)
    assert np.all(acc_flags[:, 1::8] == 0xFF) and not acc_flags[:, 0::8].any()
    assert np.all(acc_flags[:, 2::8] == 0x01) and np.all(acc_flags[:, 3::8] == 0x80)
    assert np.isnan(acc_vis.real).any() and np.isfinite(acc_vis.real).any()
    assert all((d[2] == 0).any() for d in dumps)
    products = np.abs((dumps[0][2] * np.float32(2.0**-64)) * dumps[0][0].real)
    assert ((products > 0) & (products < np.finfo(np.float32).tiny)).any()  # denormal products
    assert [int(d[1][0, 1]) for d in dumps] == [1 << d for d in range(8)]  # a bit per dump
    finite = np.abs(dumps[0][0].real[np.isfinite(dumps[0][0].real)])
    ordinary = finite[finite > 2.0**-40]
    assert ordinary.max() > 2.0**16 and ordinary.min() < 2.0**-16  # the spread of magnitudes
    assert any(d[3].any() for d in dumps) and all(d[4].any() for d in dumps)
