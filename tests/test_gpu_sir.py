"""Scale-invariant rank flag extension on the GPU (``rfi.device.ScaleInvariantRankTemplate``,
``ksp_sir``): every comparison is integer equality against
``rfi.host.ScaleInvariantRankHost``."""

import ctypes

import numpy as np
import pytest

from tests import inputs, subviews

pytestmark = pytest.mark.gpu

# Both kernels hold LEAF = 16 samples of a line in registers at a time.
# Channel-major (axis 0): a workgroup owns TILE_COLS = 128 baselines, two per lane; its 16
# wavefronts share a panel of 16 * 16 * leaves channels, leaves = 1, 2, 4, 8 or 16 (the least
# that puts all channels into one panel, so the choice changes at 256, 512, 1024, 2048
# channels); above MAX_PANEL = 4096 channels there are several panels and a forward pass.
# Transposed (axis 1): a workgroup of 256 threads takes SEGMENT = 4096 channels of one
# baseline at a time, 16 per thread; longer lines take several segments and a forward pass.
LEAF = 16
TILE_COLS = 128
PANEL_STEPS = [256, 512, 1024, 2048]
MAX_PANEL = 4096
SEGMENT = 4096

CHANNELS = sorted({1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097,
                   LEAF - 1, LEAF, LEAF + 1, 2 * MAX_PANEL - 1, 2 * MAX_PANEL, 2 * MAX_PANEL + 1}
                  | {n + d for n in PANEL_STEPS for d in (-1, 0, 1)})  # fmt: skip
BASELINES = sorted({1, 3, 15, 16, 17, 63, 64, 65, 257, TILE_COLS - 1, TILE_COLS, TILE_COLS + 1})
ETA_Q = [0, 1, 819, 1024, 2048, 4095, 4096]


@pytest.fixture(scope="module")
def context():
    from katsdpsigproc_amd import accel

    return accel.create_some_context(interactive=False)


@pytest.fixture(scope="module")
def command_queue(context):
    return context.create_command_queue()


def expected(flags, eta_q, mask=0xFF, flag_value=1):
    from katsdpsigproc_amd.rfi import host

    op = host.ScaleInvariantRankHost(eta_q / 4096.0, mask, flag_value)
    assert op.eta_q == eta_q
    return op(flags)


def sparse_flags(rs, shape, density):
    return (rs.random_sample(shape) < density).astype(np.uint8)


def add_bursts(rs, flags, count, value=1):
    """`count` runs of 1..200 channels on random baselines."""
    channels, baselines = flags.shape
    for _ in range(count):
        length = min(int(rs.randint(1, 201)), channels)
        start = rs.randint(0, channels - length + 1)
        flags[start : start + length, rs.randint(0, baselines)] |= value
    return flags


def run(context, queue, flags, eta_q, mask=0xFF, flag_value=1, transposed=False, pad=0):
    """The device operation on channel-major `flags`, every row of the buffer padded by at
    least `pad` more bytes, all padding 0xFF before the call (flags that must not count);
    checks that the padding is byte-identical afterwards. Returns channels x baselines."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import device

    channels, baselines = flags.shape
    template = device.ScaleInvariantRankTemplate(context, eta_q / 4096.0, mask, flag_value,
                                                 transposed=transposed)  # fmt: skip
    assert template.eta_q == eta_q
    fn = template.instantiate(queue, channels, baselines)
    if pad:
        dim = fn.slots["flags"].dimensions[1]
        accel.Dimension(dim.size, min_padded_size=dim.size + pad).link(dim)
    fn.ensure_all_bound()
    data = flags.T if transposed else flags
    buf = fn.buffer("flags")
    assert buf.padded_shape[1] >= data.shape[1] + pad
    padded = np.full(buf.padded_shape, 0xFF, np.uint8)
    padded[:, : data.shape[1]] = data
    queue.enqueue_write_buffer(buf.buffer, padded)
    fn()
    raw = np.empty(buf.padded_shape, np.uint8)
    queue.enqueue_read_buffer(buf.buffer, raw)
    assert np.all(raw[:, data.shape[1] :] == 0xFF), "wrote into the padding"
    out = raw[:, : data.shape[1]]
    return np.ascontiguousarray(out.T if transposed else out)


def check(context, queue, flags, eta_q, want=None, **kwargs):
    """Both layouts against the host class (or `want`, computed by the caller from it)."""
    layout = {key: kwargs.pop(key) for key in ("pad",) if key in kwargs}
    if want is None:
        want = expected(flags, eta_q, **kwargs)
    for transposed in (False, True):
        got = run(context, queue, flags, eta_q, transposed=transposed, **kwargs, **layout)
        np.testing.assert_array_equal(want, got, err_msg=f"transposed {transposed}")
    return want


@pytest.mark.parametrize("channels", CHANNELS)
def test_shapes(channels, context, command_queue):
    """Every line length with every line count, both layouts: one reference per length, whose
    first baselines are the smaller cases (lines are independent)."""
    rs = np.random.RandomState(channels)
    flags = sparse_flags(rs, (channels, BASELINES[-1]), 1.0 / 8.0)
    add_bursts(rs, flags, 20)
    want = expected(flags, 819)
    assert channels < 8 or want.sum() > flags.sum()
    for baselines in BASELINES:
        check(context, command_queue, flags[:, :baselines], 819, want=want[:, :baselines])


@pytest.fixture(scope="module")
def mixed_lines():
    """1100 channels x 150 baselines: all clear, all flagged, densities 1/64 .. 7/8, and bursts
    of 1..200 channels on a clear and on a sparse background, over more than one tile."""
    rs = np.random.RandomState(11)
    channels, baselines = 1100, 150
    flags = np.zeros((channels, baselines), np.uint8)
    flags[:, 1::7] = 1
    for k, density in enumerate((1.0 / 64.0, 1.0 / 8.0, 0.5, 7.0 / 8.0)):
        flags[:, 2 + k :: 7] = sparse_flags(rs, flags[:, 2 + k :: 7].shape, density)
    add_bursts(rs, flags[:, 6::7], 40)
    flags[:, 5::7] = sparse_flags(rs, flags[:, 5::7].shape, 1.0 / 64.0)
    add_bursts(rs, flags[:, 5::7], 40)
    assert not flags[:, 0::7].any() and flags[:, 1::7].all()
    return flags


@pytest.mark.parametrize("eta_q", ETA_Q)
def test_data_and_eta(eta_q, mixed_lines, context, command_queue):
    want = check(context, command_queue, mixed_lines, eta_q)
    assert np.all(want >= mixed_lines)
    if eta_q in (0, 1):
        # (eta_q = 1 lets one clear sample into an interval of 4096, longer than these lines)
        np.testing.assert_array_equal(want, mixed_lines)
    elif eta_q == 4096:
        assert np.all(want == 1)  # the clear lines too
    else:
        assert not want[:, 0::7].any() and want.sum() > mixed_lines.sum()


def two_blocks(channels, first, last):
    """Baselines: clear, [first flagged ... last flagged], full, the same again, clear: a
    lane that took its neighbour's sums would show."""
    line = np.zeros(channels, np.uint8)
    line[:first] = 1
    line[channels - last :] = 1
    flags = np.zeros((channels, 5), np.uint8)
    flags[:, 1] = flags[:, 3] = line
    flags[:, 2] = 1
    return flags


@pytest.mark.parametrize("channels, quarter", [(4096, 1024), (262144, 65536)])
def test_long_range(channels, quarter, context, command_queue):
    """eta = 1/2: a quarter of the line flagged at either end flags all of it (the interval
    is the whole line, an exact tie); one sample less at the far end and each block grows by
    its own length only, leaving the centre clear."""
    want = check(context, command_queue, two_blocks(channels, quarter, quarter), 2048)
    assert want[:, 1].all() and want[:, 3].all() and not want[:, 0].any() and not want[:, 4].any()
    flags = two_blocks(channels - 1, quarter, quarter - 1)
    want = check(context, command_queue, flags, 2048)
    line = np.zeros(channels - 1, np.uint8)
    line[: 2 * quarter] = 1  # the left block and exactly as many again
    line[channels - 1 - 2 * (quarter - 1) :] = 1  # the right one likewise
    assert line.sum() == channels - 2 and line[2 * quarter] == 0
    np.testing.assert_array_equal(want[:, 1], line)
    np.testing.assert_array_equal(want[:, 3], line)
    assert not want[:, 0].any() and want[:, 2].all()


def test_long_range_70000(context, command_queue):
    rs = np.random.RandomState(12)
    flags = np.zeros((70000, 3), np.uint8)
    flags[:17500, 0] = flags[-17500:, 0] = 1  # the whole line at eta = 1/2
    flags[:17500, 1] = flags[-17499:, 1] = 1  # one short of it
    flags[:, 2] = sparse_flags(rs, 70000, 1.0 / 16.0)
    add_bursts(rs, flags[:, 2:], 100)
    want = check(context, command_queue, flags, 2048)
    assert want[:, 0].all() and want[:, 1].sum() == 69998


@pytest.mark.parametrize("short", [False, True])
def test_ties_across_boundaries(short, context, command_queue):
    """eta_q = 1024: 8 flagged, 4 clear, 4 flagged is 12 of 16, 4096 * 12 == 3072 * 16. The
    block of 8 alone reaches 2 samples into the gap and the block of 4 one; the last sample
    of the gap is flagged by the interval of all 16 only, an exact tie. With the last flagged
    sample clear (11 of 15) it stays clear. The gap straddles a boundary of each kernel's
    pieces, one per baseline."""
    boundaries = [LEAF, 256, 2048, MAX_PANEL, MAX_PANEL + LEAF, 2 * MAX_PANEL]
    channels = 2 * MAX_PANEL + 300
    flags = np.zeros((channels, len(boundaries)), np.uint8)
    for k, b in enumerate(boundaries):
        flags[b - 10 : b - 2, k] = 1
        flags[b + 2 : b + 6 - short, k] = 1
    want = check(context, command_queue, flags, 1024)
    for k, b in enumerate(boundaries):
        gap = want[b - 2 : b + 2, k]
        assert gap.sum() == (3 if short else 4), f"boundary {b}"


@pytest.mark.parametrize("channels, baselines", [(65, 1025), (257, 17), (4097, 33)])
def test_padding(channels, baselines, context, command_queue):
    rs = np.random.RandomState(baselines)
    flags = sparse_flags(rs, (channels, baselines), 1.0 / 8.0)
    check(context, command_queue, flags, 819, pad=29)
    check(context, command_queue, flags, 2048, pad=1)


@pytest.mark.parametrize("mask, flag_value", [(0x01, 0x02), (0x80, 0x80), (0x06, 0x04),
                                              (0xFF, 0x01), (0x0F, 0xF0), (0x10, 0xFF)])  # fmt: skip
def test_masks(mask, flag_value, context, command_queue):
    rs = np.random.RandomState(mask)
    flags = rs.randint(0, 256, (1500, 131)).astype(np.uint8)
    flags[:, ::2] &= np.where(rs.random_sample((1500, 66)) < 0.8, 0xFF & ~mask, 0xFF).astype(np.uint8)
    want = check(context, command_queue, flags, 819, mask=mask, flag_value=flag_value)
    np.testing.assert_array_equal(want & (0xFF & ~flag_value), flags & (0xFF & ~flag_value))
    assert np.all(want[(flags & mask) != 0] & flag_value == flag_value)
    assert (want != flags).any()


def call_abi(context, queue, data, stride, offset, axis, eta_q, mask=0xFF, flag_value=1,
             views=None):
    """ksp_sir on `data` (as it lies in memory) with `stride` bytes per row, `offset` bytes
    into an allocation full of sentinels (0xAB: flags that must not count). `views` makes the
    array (subviews.CompactViews unless given) and may choose another stride."""
    from katsdpsigproc_amd import _lib

    view = (views or subviews.CompactViews(context, queue))("flags", np.uint8, data, stride, offset)[0]
    _lib.call("ksp_sir", context.device.index, ctypes.c_void_p(queue.stream), view.ptr,
              data.shape[0], data.shape[1], view.stride, axis, eta_q, mask, flag_value)  # fmt: skip
    return view.read("flags")


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("offset", [0, 1, 12])
@pytest.mark.parametrize("stride", [1003, 1007])
def test_subviews(stride, offset, axis, context, command_queue):
    rs = np.random.RandomState(stride + offset)
    data = rs.randint(0, 256, (37, 1003)).astype(np.uint8)
    data &= np.where(rs.random_sample(data.shape) < 0.85, 0xFE, 0xFF).astype(np.uint8)
    got = call_abi(context, command_queue, data, stride, offset, axis, 819, mask=0x01, flag_value=0x03)
    lines = data if axis == 0 else data.T
    want = expected(lines, 819, 0x01, 0x03)
    np.testing.assert_array_equal(want if axis == 0 else want.T, got)
    assert (got != data).any()


def test_behind_the_flagger(context, command_queue):
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import device, host

    channels, baselines = 64, 40
    rs = np.random.RandomState(13)
    vis = inputs.generate_data(channels, baselines, seed=5)
    spikes = rs.random_sample(vis.shape) < 1.0 / 16.0
    vis[spikes] += np.complex64(60.0)
    vis[20:26, 8:24] += np.complex64(40.0 + 40.0j)  # a broadband burst on 16 baselines
    args = {"n_sigma": 11.0}
    template = device.FlaggerDeviceTemplate(
        device.BackgroundMedianFilterDeviceTemplate(context, 13),
        device.NoiseEstMADTDeviceTemplate(context, channels),
        device.ThresholdSumDeviceTemplate(context, flag_value=4),
    )
    flagger = template.instantiate(command_queue, channels, baselines, threshold_args=args)
    assert isinstance(flagger, device.FusedFlaggerDevice)
    sir = device.ScaleInvariantRankTemplate(context, 0.2, mask=4, flag_value=8).instantiate(
        command_queue, channels, baselines)
    masks = (0x04, 0x08, 0x0C)
    count = device.FlagCountTemplate(context, masks).instantiate(command_queue, channels, baselines)
    seq = accel.OperationSequence(
        command_queue, [("flagger", flagger), ("sir", sir), ("count", count)],
        compounds={"flags": ["flagger:flags", "sir:flags", "count:flags"]})  # fmt: skip
    seq.ensure_all_bound()
    seq.buffer("flagger:vis").set(command_queue, vis)
    seq()
    flags = seq.buffer("flags").get(command_queue)
    host_flagger = host.FlaggerHost(host.BackgroundMedianFilterHost(13), host.NoiseEstMADHost(),
                                    host.ThresholdSumHost(11.0, flag_value=4))  # fmt: skip
    detected = host_flagger(vis)
    want = host.ScaleInvariantRankHost(0.2, mask=4, flag_value=8)(detected)
    np.testing.assert_array_equal(want, flags)
    assert detected.any() and (want != detected).any()
    want_c, want_b = host.FlagCountHost(masks)(want)
    channel_counts = seq.buffer("count:channel_counts").get(command_queue)
    np.testing.assert_array_equal(want_c, channel_counts)
    np.testing.assert_array_equal(want_b, seq.buffer("count:baseline_counts").get(command_queue))
    assert channel_counts[1].sum() > channel_counts[0].sum() > 0  # extended beyond detected
    np.testing.assert_array_equal(channel_counts[1], channel_counts[2])


@pytest.mark.parametrize("transposed", [False, True])
def test_host_from_device(transposed, context, command_queue):
    from katsdpsigproc_amd.rfi import device

    rs = np.random.RandomState(9)
    flags = add_bursts(rs, sparse_flags(rs, (117, 273), 1.0 / 16.0), 30, value=0x20)
    template = device.ScaleInvariantRankTemplate(context, 0.3, mask=0x21, flag_value=0x40,
                                                 transposed=transposed)  # fmt: skip
    before = flags.copy()
    got = device.ScaleInvariantRankHostFromDevice(template, command_queue)(flags)
    np.testing.assert_array_equal(before, flags)  # a new array
    np.testing.assert_array_equal(template.host_class(0.3, mask=0x21, flag_value=0x40)(flags), got)
    assert got.shape == flags.shape and got.dtype == np.uint8
