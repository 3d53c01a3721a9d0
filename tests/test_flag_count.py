"""Flag counting without a GPU: the NumPy class against a double loop, argument errors,
slot wiring on the fake backend, composition behind the fused flagger, and the argument
checks of ``ksp_flag_count``, which come before any device call."""

import ctypes

import numpy as np
import pytest

from katsdpsigproc_amd import accel
from katsdpsigproc_amd.rfi import device, host
from tests.fakes import FakeContext

MASKS = (0xFF, 0x01, 0x80, 0x81)


@pytest.fixture
def context():
    return FakeContext()


@pytest.fixture
def queue(context):
    return context.create_command_queue()


def test_host_against_double_loop():
    rs = np.random.RandomState(5)
    flags = rs.randint(0, 256, (13, 9)).astype(np.uint8)
    channel_counts, baseline_counts = host.FlagCountHost(MASKS)(flags)
    assert channel_counts.dtype == np.uint32 and channel_counts.shape == (4, 13)
    assert baseline_counts.dtype == np.uint32 and baseline_counts.shape == (4, 9)
    for m, mask in enumerate(MASKS):
        for c in range(13):
            assert channel_counts[m, c] == sum(1 for b in range(9) if int(flags[c, b]) & mask)
        for b in range(9):
            assert baseline_counts[m, b] == sum(1 for c in range(13) if int(flags[c, b]) & mask)
    # the default counts any flag
    any_c, any_b = host.FlagCountHost()(flags)
    np.testing.assert_array_equal(any_c, channel_counts[:1])
    np.testing.assert_array_equal(any_b, baseline_counts[:1])
    assert 0 < any_c.sum() == any_b.sum() == np.count_nonzero(flags)


@pytest.mark.parametrize("make", [
    lambda masks: host.FlagCountHost(masks),
    lambda masks: device.FlagCountTemplate(FakeContext(), masks),
], ids=["host", "template"])  # fmt: skip
def test_mask_errors(make):
    for bad in [(), (1,) * 9, (0,), (256,), (1, -1), (0xFF, 300)]:
        with pytest.raises(ValueError):
            make(bad)
    for bad in [(1.0,), ("1",), (None,), (True,)]:
        with pytest.raises(TypeError):
            make(bad)
    assert make((np.uint8(3), 255)).masks == (3, 255)
    assert make([1, 2, 4, 8, 16, 32, 64, 128]).masks == (1, 2, 4, 8, 16, 32, 64, 128)


def test_template_errors(context, queue):
    template = device.FlagCountTemplate(context)
    for channels, baselines in [(0, 4), (4, 0), (-1, 4)]:
        with pytest.raises(ValueError):
            template.instantiate(queue, channels, baselines)
    with pytest.raises(ValueError):
        device.FlagCountTemplate(context, tuning={"wgs": 256})
    assert device.FlagCountTemplate(context, tuning={}).tuning == {}
    assert device.FlagCountTemplate.autotune(context) == {}
    with pytest.raises(ValueError):
        device.FlagCountHostFromDevice(device.FlagCountTemplate(context, accumulate=True), queue)


@pytest.mark.parametrize("transposed", [False, True])
def test_wiring(transposed, context, queue):
    template = device.FlagCountTemplate(context, MASKS, transposed=transposed)
    fn = template.instantiate(queue, 300, 200)
    assert set(fn.slots) == {"flags", "channel_counts", "baseline_counts"}
    assert fn.slots["flags"].shape == ((200, 300) if transposed else (300, 200))
    assert fn.slots["flags"].dtype == np.uint8
    assert fn.slots["channel_counts"].shape == (4, 300)
    assert fn.slots["baseline_counts"].shape == (4, 200)
    assert fn.slots["channel_counts"].dtype == fn.slots["baseline_counts"].dtype == np.uint32
    fn()
    assert [name for name, _ in queue.launches] == ["ksp_flag_count"]
    args = queue.launches[0][1]
    rows_of = "baseline_counts" if transposed else "channel_counts"
    cols_of = "channel_counts" if transposed else "baseline_counts"
    assert args[0] is fn.buffer("flags").buffer
    assert args[1] is fn.buffer(rows_of).buffer and args[2] is fn.buffer(cols_of).buffer
    # rows, cols, then the padded strides of the three slots (128-byte rows)
    rows, cols = (200, 300) if transposed else (300, 200)
    assert [int(a) for a in args[3:8]] == [
        rows, cols, fn.buffer("flags").padded_shape[1],
        fn.buffer(rows_of).padded_shape[1], fn.buffer(cols_of).padded_shape[1]]  # fmt: skip
    assert fn.buffer("flags").padded_shape[1] == (384 if transposed else 256)
    assert fn.buffer("channel_counts").padded_shape == (4, 320)
    assert fn.buffer("baseline_counts").padded_shape == (4, 224)
    assert list(args[8]) == list(MASKS) and int(args[9]) == 4 and int(args[10]) == 0
    assert fn.parameters() == {"masks": MASKS, "transposed": transposed, "accumulate": False,
                               "channels": 300, "baselines": 200}  # fmt: skip
    acc = device.FlagCountTemplate(context, accumulate=True).instantiate(queue, 5, 7)
    acc()
    assert int(queue.launches[-1][1][10]) == 1 and acc.parameters()["accumulate"] is True
    assert list(queue.launches[-1][1][8]) == [0xFF]


def test_behind_the_fused_flagger(context, queue):
    flagger = device.FlaggerDeviceTemplate(
        device.BackgroundMedianFilterDeviceTemplate(context, 13),
        device.NoiseEstMADTDeviceTemplate(context, 4096),
        device.ThresholdSumDeviceTemplate(context),
        tuning={"vis_pad": 0},
    ).instantiate(queue, 4096, 200, threshold_args={"n_sigma": 11.0})
    assert isinstance(flagger, device.FusedFlaggerDevice)
    count = device.FlagCountTemplate(context).instantiate(queue, 4096, 200)
    # some more row padding than either asks for, as a caller's own requirement would
    dim = flagger.slots["flags"].dimensions[1]
    accel.Dimension(200, min_padded_size=300).link(dim)
    seq = accel.OperationSequence(queue, [("flagger", flagger), ("count", count)],
                                  compounds={"flags": ["flagger:flags", "count:flags"]})  # fmt: skip
    assert "flagger:flags" not in seq.slots and "count:flags" not in seq.slots
    assert seq.slots["flags"].shape == (4096, 200)
    # a sequence allocates every slot it shows, the flagger's optional temporaries included
    # (which then get computed); a caller who does not want them takes them off the list
    for name in device.FusedFlaggerDevice._OPTIONAL:
        del seq.slots["flagger:" + name]
    seq()
    assert [name for name, _ in queue.launches] == ["ksp_flagger_fused", "ksp_flag_count"]
    assert queue.launches[0][1][3] is None  # no deviations asked of the kernel
    assert flagger.buffer("flags") is count.buffer("flags") is seq.buffer("flags")
    padded = seq.buffer("flags").padded_shape[1]
    assert padded == 384  # 300 rounded up to 128-byte rows: one size for both operations
    assert int(queue.launches[0][1][9]) == padded  # the flagger's flags stride
    assert int(queue.launches[1][1][5]) == padded  # the counter's
    # linking after the fact is refused: the dimensions are frozen by the binding
    with pytest.raises(ValueError):
        accel.Dimension(200).link(count.slots["flags"].dimensions[1])


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
    one = (ctypes.c_uint8 * 9)(*([1] * 9))

    def call(flags=p, row_counts=p, col_counts=p, rows=4, cols=8, stride=8, rstride=4,
             cstride=8, masks=one, n_masks=1, accumulate=0):  # fmt: skip
        rc = lib.ksp_flag_count(0, None, flags, row_counts, col_counts, rows, cols, stride,
                                rstride, cstride, masks, n_masks, accumulate)  # fmt: skip
        assert rc != 0
        return _lib.last_error()

    assert "invalid argument: flags is NULL" in call(flags=None)
    assert "invalid argument: row_counts is NULL" in call(row_counts=None)
    assert "invalid argument: col_counts is NULL" in call(col_counts=None)
    assert "invalid argument: masks is NULL" in call(masks=None)
    assert "rows" in call(rows=0)
    assert "cols" in call(cols=0)
    assert "invalid argument: stride is smaller than cols" in call(stride=7)
    assert "invalid argument: row_counts_stride is smaller than rows" in call(rstride=3)
    assert "invalid argument: col_counts_stride is smaller than cols" in call(cstride=7)
    assert "n_masks" in call(n_masks=0)
    assert "n_masks" in call(n_masks=9)
    assert "mask is zero" in call(masks=(ctypes.c_uint8 * 2)(1, 0), n_masks=2)
