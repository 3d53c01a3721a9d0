"""Scale-invariant rank flag extension without a GPU: the NumPy class against the interval
definition, its properties and errors, slot wiring on the fake backend, composition between
the fused flagger and the flag counter, and the argument checks of ``ksp_sir``, which come
before any device call."""

import ctypes

import numpy as np
import pytest

from katsdpsigproc_amd import accel
from katsdpsigproc_amd.rfi import device, host
from tests.fakes import FakeContext

ETA_Q = (0, 1, 819, 2048, 4095, 4096)
DENSITIES = (0.0, 0.05, 0.3, 0.9, 1.0)


@pytest.fixture
def context():
    return FakeContext()


@pytest.fixture
def queue(context):
    return context.create_command_queue()


def brute_force(flagged, eta_q):
    """The interval definition on one line of booleans: every sample of every [a, b) with
    4096 * #flagged >= (4096 - eta_q) * (b - a)."""
    n = len(flagged)
    result = np.zeros(n, bool)
    count = np.concatenate([[0], np.cumsum(flagged)])
    for a in range(n):
        for b in range(a + 1, n + 1):
            if 4096 * (count[b] - count[a]) >= (4096 - eta_q) * (b - a):
                result[a:b] = True
    return result


def with_eta_q(eta_q, **kwargs):
    op = host.ScaleInvariantRankHost(eta_q / 4096.0, **kwargs)
    assert op.eta_q == eta_q
    return op


@pytest.mark.parametrize("eta_q", ETA_Q)
def test_host_against_intervals(eta_q):
    rs = np.random.RandomState(eta_q)
    for n in (1, 2, 3, 7, 33, 64):
        flags = np.stack([(rs.random_sample(n) < d).astype(np.uint8) for d in DENSITIES], axis=1)
        out = with_eta_q(eta_q)(flags)
        assert out.dtype == np.uint8 and out.shape == flags.shape and out is not flags
        for line in range(len(DENSITIES)):
            want = brute_force(flags[:, line] != 0, eta_q)
            np.testing.assert_array_equal(want, out[:, line] != 0, err_msg=f"n {n}, line {line}")


@pytest.mark.parametrize("mask", [0x01, 0x80, 0x06])
def test_host_masks_on_random_bytes(mask):
    rs = np.random.RandomState(mask)
    flags = rs.randint(1, 256, (48, 6)).astype(np.uint8)
    for eta_q in (819, 2048):
        out = with_eta_q(eta_q, mask=mask, flag_value=0x40)(flags)
        for line in range(flags.shape[1]):
            want = brute_force((flags[:, line] & mask) != 0, eta_q)
            np.testing.assert_array_equal(
                flags[:, line] | np.where(want, 0x40, 0).astype(np.uint8), out[:, line])


def test_host_properties():
    rs = np.random.RandomState(2)
    flags = (rs.random_sample((200, 9)) < 0.2).astype(np.uint8)
    flags[:, 0] = 0  # an empty line
    flags[:, 1] = 1  # a full one
    for eta_q in ETA_Q:
        out = with_eta_q(eta_q)(flags)
        assert np.all(out >= flags)  # the result contains the input
    np.testing.assert_array_equal(flags, with_eta_q(0)(flags))
    assert np.all(with_eta_q(4096)(flags) == 1)  # empty lines too
    # monotone in eta
    low, high = with_eta_q(819)(flags), with_eta_q(2048)(flags)
    assert np.all(high >= low) and high.sum() > low.sum() > flags.sum()


def test_host_quantisation():
    assert host.ScaleInvariantRankHost(0.2).eta_q == 819
    assert host.ScaleInvariantRankHost(0.25).eta_q == 1024
    assert host.ScaleInvariantRankHost(0.5 / 4096).eta_q == 1  # the half rounds up
    assert host.ScaleInvariantRankHost(0.49 / 4096).eta_q == 0
    assert host.ScaleInvariantRankHost(0).eta_q == 0
    assert host.ScaleInvariantRankHost(1).eta_q == 4096
    assert host.ScaleInvariantRankHost(np.float32(0.5)).eta_q == 2048


def test_host_exact_tie():
    line = np.array([[1, 1, 0, 1, 0, 0, 0, 0]], np.uint8).T
    # [0, 4): 3 of 4 flagged, 4096 * 3 == (4096 - 1024) * 4
    np.testing.assert_array_equal(
        host.ScaleInvariantRankHost(0.25)(line)[:, 0], [1, 1, 1, 1, 0, 0, 0, 0])
    np.testing.assert_array_equal(with_eta_q(1023)(line), line)


def test_host_bits():
    rs = np.random.RandomState(3)
    flags = rs.randint(0, 256, (64, 5)).astype(np.uint8)
    # flag_value outside the mask: "extended only" is bit 1 without bit 0
    out = host.ScaleInvariantRankHost(0.3, mask=1, flag_value=2)(flags & 0xFD)
    np.testing.assert_array_equal(out & 0xFD, flags & 0xFD)  # every other bit is kept
    assert np.all((out & 2) >> 1 >= out & 1)  # a sample flagged under the mask gets it too
    assert np.any((out & 3) == 2)
    for line in range(5):
        np.testing.assert_array_equal(brute_force((flags[:, line] & 1) != 0, 1229),
                                      (out[:, line] & 2) != 0)
    # flag_value inside the mask: what is written never counts as input
    inside = host.ScaleInvariantRankHost(0.3, mask=3, flag_value=2)(flags)
    for line in range(5):
        np.testing.assert_array_equal(
            flags[:, line] | np.where(brute_force((flags[:, line] & 3) != 0, 1229), 2, 0),
            inside[:, line])
    np.testing.assert_array_equal(inside & 0xFD, flags & 0xFD)
    with pytest.raises(ValueError):
        host.ScaleInvariantRankHost(0.3)(flags.astype(np.int32))
    with pytest.raises(ValueError):
        host.ScaleInvariantRankHost(0.3)(flags[0])


@pytest.mark.parametrize("make", [
    lambda *args, **kwargs: host.ScaleInvariantRankHost(*args, **kwargs),
    lambda *args, **kwargs: device.ScaleInvariantRankTemplate(FakeContext(), *args, **kwargs),
], ids=["host", "template"])  # fmt: skip
def test_parameter_errors(make):
    for eta in (-0.001, 1.001, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            make(eta)
    for name in ("mask", "flag_value"):
        for bad in (0, 256, -1):
            with pytest.raises(ValueError):
                make(0.2, **{name: bad})
        for bad in (1.0, "1", None, True):
            with pytest.raises(TypeError):
                make(0.2, **{name: bad})
    op = make(0.2, mask=np.uint8(6), flag_value=np.int64(255))
    assert (op.eta_q, op.mask, op.flag_value) == (819, 6, 255)
    assert type(op.mask) is int and type(op.flag_value) is int
    assert (make(0.2).mask, make(0.2).flag_value) == (0xFF, 1)


def test_template_errors(context, queue):
    template = device.ScaleInvariantRankTemplate(context, 0.2)
    assert template.host_class is host.ScaleInvariantRankHost
    for channels, baselines in [(0, 4), (4, 0), (-1, 4), (262145, 4)]:
        with pytest.raises(ValueError):
            template.instantiate(queue, channels, baselines)
    template.instantiate(queue, 262144, 1)
    template.instantiate(queue, 1, 300000)  # only channels are limited
    with pytest.raises(ValueError):
        device.ScaleInvariantRankTemplate(context, 0.2, tuning={"wgs": 256})
    assert device.ScaleInvariantRankTemplate(context, 0.2, tuning={}).tuning == {}
    assert device.ScaleInvariantRankTemplate.autotune(context) == {}


@pytest.mark.parametrize("transposed", [False, True])
def test_wiring(transposed, context, queue):
    template = device.ScaleInvariantRankTemplate(context, 0.2, mask=0x0F, flag_value=0x10,
                                                 transposed=transposed)  # fmt: skip
    fn = template.instantiate(queue, 300, 200)
    assert set(fn.slots) == {"flags"}
    assert fn.slots["flags"].shape == ((200, 300) if transposed else (300, 200))
    assert fn.slots["flags"].dtype == np.uint8
    fn()
    assert [name for name, _ in queue.launches] == ["ksp_sir"]
    args = queue.launches[0][1]
    assert args[0] is fn.buffer("flags").buffer
    rows, cols = (200, 300) if transposed else (300, 200)
    # rows, cols, the padded stride (128-byte rows), the axis of the lines, eta_q, mask, value
    assert fn.buffer("flags").padded_shape[1] == (384 if transposed else 256)
    assert [int(a) for a in args[1:]] == [
        rows, cols, fn.buffer("flags").padded_shape[1], int(transposed), 819, 0x0F, 0x10]
    assert len(args) == 8
    assert fn.parameters() == {"eta_q": 819, "mask": 0x0F, "flag_value": 0x10,
                               "transposed": transposed, "channels": 300, "baselines": 200}  # fmt: skip


def test_wiring_padded(context, queue):
    """A caller's own row padding reaches the launcher as the stride."""
    fn = device.ScaleInvariantRankTemplate(context, 1.0).instantiate(queue, 5, 7)
    dim = fn.slots["flags"].dimensions[1]
    accel.Dimension(7, min_padded_size=300).link(dim)
    fn()
    assert fn.buffer("flags").padded_shape == (5, 384)
    assert [int(a) for a in queue.launches[0][1][1:]] == [5, 7, 384, 0, 4096, 0xFF, 1]


def test_between_flagger_and_count(context, queue):
    flagger = device.FlaggerDeviceTemplate(
        device.BackgroundMedianFilterDeviceTemplate(context, 13),
        device.NoiseEstMADTDeviceTemplate(context, 4096),
        device.ThresholdSumDeviceTemplate(context),
        tuning={"vis_pad": 0},
    ).instantiate(queue, 4096, 200, threshold_args={"n_sigma": 11.0})
    assert isinstance(flagger, device.FusedFlaggerDevice)
    sir = device.ScaleInvariantRankTemplate(context, 0.2).instantiate(queue, 4096, 200)
    count = device.FlagCountTemplate(context).instantiate(queue, 4096, 200)
    accel.Dimension(200, min_padded_size=300).link(flagger.slots["flags"].dimensions[1])
    seq = accel.OperationSequence(
        queue, [("flagger", flagger), ("sir", sir), ("count", count)],
        compounds={"flags": ["flagger:flags", "sir:flags", "count:flags"]})  # fmt: skip
    assert not {"flagger:flags", "sir:flags", "count:flags"} & set(seq.slots)
    assert seq.slots["flags"].shape == (4096, 200)
    for name in device.FusedFlaggerDevice._OPTIONAL:
        del seq.slots["flagger:" + name]
    seq()
    assert [name for name, _ in queue.launches] == ["ksp_flagger_fused", "ksp_sir", "ksp_flag_count"]
    assert flagger.buffer("flags") is sir.buffer("flags") is count.buffer("flags")
    assert seq.buffer("flags") is sir.buffer("flags")
    padded = seq.buffer("flags").padded_shape[1]
    assert padded == 384  # one size for all three
    assert int(queue.launches[0][1][9]) == padded  # the flagger's flags stride
    assert queue.launches[1][1][0] is seq.buffer("flags").buffer
    assert [int(a) for a in queue.launches[1][1][1:4]] == [4096, 200, padded]
    assert int(queue.launches[2][1][5]) == padded  # the counter's


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

    def call(flags=p, rows=4, cols=8, stride=8, axis=0, eta_q=819, mask=0xFF, flag_value=1):
        rc = lib.ksp_sir(0, None, flags, rows, cols, stride, axis, eta_q, mask, flag_value)
        assert rc != 0
        return _lib.last_error()

    assert "invalid argument: flags is NULL" in call(flags=None)
    assert "axis" in call(axis=2)
    assert "axis" in call(axis=-1)
    assert "rows" in call(rows=0)
    assert "cols" in call(cols=0)
    assert "invalid argument: stride is smaller than cols" in call(stride=7)
    assert "262144" in call(rows=262145, axis=0)
    assert "262144" in call(cols=262145, stride=262145, axis=1)
    assert "eta_q" in call(eta_q=-1)
    assert "eta_q" in call(eta_q=4097)
    assert "mask" in call(mask=0)
    assert "mask" in call(mask=256)
    assert "flag_value" in call(flag_value=0)
    assert "flag_value" in call(flag_value=256)
