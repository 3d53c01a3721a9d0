"""Flag counts per channel and per baseline on the GPU (``rfi.device.FlagCountTemplate``,
``ksp_flag_count``): every comparison is exact, against ``rfi.host.FlagCountHost``."""

import ctypes

import numpy as np
import pytest

from tests import inputs, subviews

pytestmark = pytest.mark.gpu

# The kernel's tile is 4096 columns wide (256 lanes x 16 bytes, 1024 per wavefront) and
# min(max(8 * ceil(rows * ceil(cols / 4096) / 1024 / 8), 32 or, with several masks, 64), 128)
# rows high, walked 8 rows at a time: 32 rows for every small array below, 128 for the tall
# ones of test_tall_tiles.
TILE_COLS = 4096
MIN_TILE_ROWS = 32
MAX_TILE_ROWS = 128
ROWS = [1, 2, 63, 64, 65, 257, MIN_TILE_ROWS - 1, MIN_TILE_ROWS, MIN_TILE_ROWS + 1,
        MAX_TILE_ROWS - 1, MAX_TILE_ROWS, MAX_TILE_ROWS + 1]  # fmt: skip
COLS = [1, 15, 16, 17, 1023, 1024, 1025, 4097, TILE_COLS - 1, TILE_COLS]


@pytest.fixture(scope="module")
def context():
    from katsdpsigproc_amd import accel

    return accel.create_some_context(interactive=False)


@pytest.fixture(scope="module")
def command_queue(context):
    return context.create_command_queue()


def sparse_flags(rs, shape, density=1.0 / 8.0):
    """Bytes that are 0 with probability 1 - density, else uniform in 1..255."""
    values = rs.randint(1, 256, shape).astype(np.uint8)
    return np.where(rs.random_sample(shape) < density, values, np.uint8(0))


def expected(flags, masks):
    from katsdpsigproc_amd.rfi import host

    return host.FlagCountHost(masks)(flags)


def read_padded(queue, array):
    raw = np.empty(array.padded_shape, array.dtype)
    queue.enqueue_read_buffer(array.buffer, raw)
    return raw


def run(context, queue, flags, masks=(0xFF,), transposed=False, pad=0):
    """(channel_counts, baseline_counts) of channel-major `flags` from the device operation,
    every row padded by at least `pad` more elements; checks that the padding of the outputs
    is left alone."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import device

    channels, baselines = flags.shape
    fn = device.FlagCountTemplate(context, masks, transposed=transposed).instantiate(
        queue, channels, baselines)  # fmt: skip
    if pad:
        for name in ("flags", "channel_counts", "baseline_counts"):
            dim = fn.slots[name].dimensions[1]
            accel.Dimension(dim.size, min_padded_size=dim.size + pad).link(dim)
    fn.ensure_all_bound()
    data = flags.T if transposed else flags
    buf = fn.buffer("flags")
    assert buf.padded_shape[1] >= data.shape[1] + pad
    padded = np.full(buf.padded_shape, 0xFF, np.uint8)  # flags in the padding: never counted
    padded[:, : data.shape[1]] = data
    queue.enqueue_write_buffer(buf.buffer, padded)
    for name in ("channel_counts", "baseline_counts"):
        out = fn.buffer(name)
        queue.enqueue_write_buffer(out.buffer, np.full(out.padded_shape, 0xABABABAB, np.uint32))
    fn()
    result = []
    for name in ("channel_counts", "baseline_counts"):
        out = fn.buffer(name)
        raw = read_padded(queue, out)
        assert np.all(raw[:, out.shape[1] :] == 0xABABABAB), f"wrote into the padding of {name}"
        result.append(np.ascontiguousarray(raw[:, : out.shape[1]]))
    return result


def check(context, queue, flags, masks=(0xFF,), **kwargs):
    channel_counts, baseline_counts = run(context, queue, flags, masks, **kwargs)
    want_c, want_b = expected(flags, masks)
    np.testing.assert_array_equal(want_c, channel_counts)
    np.testing.assert_array_equal(want_b, baseline_counts)
    assert channel_counts.dtype == baseline_counts.dtype == np.uint32
    return channel_counts, baseline_counts


@pytest.mark.parametrize("rows", ROWS)
def test_shapes(rows, context, command_queue):
    rs = np.random.RandomState(rows)
    for cols in COLS:
        check(context, command_queue, sparse_flags(rs, (rows, cols)))


@pytest.mark.parametrize("rows, cols", [(131071, 16), (131072, 16), (131073, 17)])
def test_tall_tiles(rows, cols, context, command_queue):
    """Enough rows for tiles of 128: the packed byte counters of a column see 128 rows, and
    the last tile is one row short, full, or holds a single row."""
    rs = np.random.RandomState(cols)
    flags = sparse_flags(rs, (rows, cols), 0.5)
    flags[1000:1400] = 0xFF  # columns that count every row of their tiles
    check(context, command_queue, flags)


@pytest.mark.parametrize("rows, cols", [(65, 1025), (257, 17), (33, 4097)])
def test_padding(rows, cols, context, command_queue):
    flags = sparse_flags(np.random.RandomState(1), (rows, cols))
    check(context, command_queue, flags, pad=29)
    check(context, command_queue, flags, (0x0F, 0x80), pad=29, transposed=True)


def call_abi(context, queue, flags, stride, offset, masks=(0xFF,), views=None):
    """ksp_flag_count on `flags` laid out with `stride` bytes per row, starting `offset`
    bytes into an allocation; the outputs have stride rows + 3 / cols + 5. `views` makes the
    arrays (subviews.CompactViews unless given) and may choose other strides."""
    from katsdpsigproc_amd import _lib

    views = views or subviews.CompactViews(context, queue)
    rows, cols = flags.shape
    dev_in = views("flags", np.uint8, flags, stride, offset, poison=True)[0]
    blank = subviews.sentinel_array  # (counts start as sentinels: the launcher overwrites them)
    row_out = views("row_counts", np.uint32, blank((len(masks), rows), np.uint32), rows + 3)[0]
    col_out = views("col_counts", np.uint32, blank((len(masks), cols), np.uint32), cols + 5)[0]
    _lib.call("ksp_flag_count", context.device.index, ctypes.c_void_p(queue.stream),
              dev_in.ptr, row_out.ptr, col_out.ptr, rows, cols, dev_in.stride, row_out.stride,
              col_out.stride, (ctypes.c_uint8 * len(masks))(*masks), len(masks), 0)  # fmt: skip
    dev_in.read("flags")
    return row_out.read("row_counts"), col_out.read("col_counts")


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("stride", [1003, 1007])
def test_unaligned(stride, offset, context, command_queue):
    flags = sparse_flags(np.random.RandomState(stride), (37, 1003))
    masks = (0xFF, 0x10)
    row_counts, col_counts = call_abi(context, command_queue, flags, stride, offset, masks)
    want_rows, want_cols = expected(flags, masks)
    np.testing.assert_array_equal(want_rows, row_counts)
    np.testing.assert_array_equal(want_cols, col_counts)


def test_saturation(context, command_queue):
    """More rows / columns than a byte or 16 bits can count, every sample flagged."""
    channel_counts, baseline_counts = check(
        context, command_queue, np.full((70000, 24), 0xFF, np.uint8))
    assert np.all(baseline_counts == 70000) and np.all(channel_counts == 24)
    channel_counts, baseline_counts = check(
        context, command_queue, np.full((3, 70000), 0xFF, np.uint8))
    assert np.all(channel_counts == 70000) and np.all(baseline_counts == 3)
    channel_counts, baseline_counts = check(
        context, command_queue, np.full((300, 4096), 0x80, np.uint8), (0x80, 0x7F))
    assert np.all(channel_counts[0] == 4096) and np.all(baseline_counts[0] == 300)
    assert not channel_counts[1].any() and not baseline_counts[1].any()


@pytest.mark.parametrize("masks", [(1, 2, 4, 8, 16, 32, 64, 128),
                                   (0xFF, 0x0F, 0xF0, 0x81, 0x80, 0x01, 0x7E, 0x18)])  # fmt: skip
def test_masks(masks, context, command_queue):
    flags = np.random.RandomState(7).randint(0, 256, (257, 1025)).astype(np.uint8)
    for n_masks in range(1, 9):  # every kernel instantiation; all 8 masks last
        check(context, command_queue, flags, masks[:n_masks])
    check(context, command_queue, flags, masks[2:7])


def test_accumulate(context, command_queue):
    from katsdpsigproc_amd.rfi import device

    rs = np.random.RandomState(3)
    masks = (0xFF, 0x04)
    arrays = [sparse_flags(rs, (130, 1030), d) for d in (0.1, 0.5, 0.9)]
    fn = device.FlagCountTemplate(context, masks, accumulate=True).instantiate(
        command_queue, 130, 1030)
    fn.ensure_all_bound()
    fn.buffer("channel_counts").zero(command_queue)
    fn.buffer("baseline_counts").zero(command_queue)
    for flags in arrays:
        fn.buffer("flags").set(command_queue, flags)
        fn()
    want = [expected(flags, masks) for flags in arrays]
    np.testing.assert_array_equal(sum(w[0] for w in want), fn.buffer("channel_counts").get(command_queue))
    np.testing.assert_array_equal(sum(w[1] for w in want), fn.buffer("baseline_counts").get(command_queue))
    # the sums wrap modulo 2**32
    start = np.full((2, 130), 0xFFFFFFF0, np.uint32)
    fn.buffer("channel_counts").set(command_queue, start)
    fn()
    np.testing.assert_array_equal(start + want[2][0],
                                  fn.buffer("channel_counts").get(command_queue))  # fmt: skip
    assert np.all(start + want[2][0] < start)  # every counter did wrap
    # without accumulate whatever the outputs held is overwritten (run() poisons them)
    check(context, command_queue, arrays[0], masks)


def test_transposed(context, command_queue):
    flags = sparse_flags(np.random.RandomState(4), (300, 1100))
    masks = (0xFF, 0x21)
    plain = run(context, command_queue, flags, masks)
    transposed = run(context, command_queue, flags, masks, transposed=True)
    assert plain[0].shape == (2, 300) and plain[1].shape == (2, 1100)
    np.testing.assert_array_equal(plain[0], transposed[0])
    np.testing.assert_array_equal(plain[1], transposed[1])
    np.testing.assert_array_equal(expected(flags, masks)[0], plain[0])


@pytest.mark.parametrize("shape", [(4096, 2048), (2048, 4096)])
def test_many_workgroups(shape, context, command_queue):
    flags = sparse_flags(np.random.RandomState(8), shape, 1.0 / 16.0)
    check(context, command_queue, flags, (0xFF, 0x02))


def test_behind_the_flagger(context, command_queue):
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import device

    channels, baselines = 256, 96
    vis = inputs.add_rfi(inputs.generate_data(channels, baselines, seed=5), seed=6)
    template = device.FlaggerDeviceTemplate(
        device.BackgroundMedianFilterDeviceTemplate(context, 13),
        device.NoiseEstMADTDeviceTemplate(context, channels),
        device.ThresholdSumDeviceTemplate(context, flag_value=4),
    )
    args = {"n_sigma": 11.0}
    alone = device.FlaggerHostFromDevice(template, command_queue, threshold_args=args)(vis)
    flagger = template.instantiate(command_queue, channels, baselines, threshold_args=args)
    masks = (0xFF, 0x04, 0x01)
    count = device.FlagCountTemplate(context, masks).instantiate(command_queue, channels, baselines)
    seq = accel.OperationSequence(command_queue, [("flagger", flagger), ("count", count)],
                                  compounds={"flags": ["flagger:flags", "count:flags"]})  # fmt: skip
    seq.ensure_all_bound()
    seq.buffer("flagger:vis").set(command_queue, vis)
    seq()
    flags = seq.buffer("flags").get(command_queue)
    np.testing.assert_array_equal(alone, flags)
    want_c, want_b = expected(flags, masks)
    channel_counts = seq.buffer("count:channel_counts").get(command_queue)
    np.testing.assert_array_equal(want_c, channel_counts)
    np.testing.assert_array_equal(want_b, seq.buffer("count:baseline_counts").get(command_queue))
    assert channel_counts[0].sum() > 0 and not channel_counts[2].any()
    np.testing.assert_array_equal(channel_counts[0], channel_counts[1])


@pytest.mark.parametrize("transposed", [False, True])
def test_host_from_device(transposed, context, command_queue):
    from katsdpsigproc_amd.rfi import device

    flags = sparse_flags(np.random.RandomState(9), (117, 273))
    masks = (0xFF, 0x40, 0x03)
    template = device.FlagCountTemplate(context, masks, transposed=transposed)
    channel_counts, baseline_counts = device.FlagCountHostFromDevice(template, command_queue)(flags)
    want_c, want_b = expected(flags, masks)
    np.testing.assert_array_equal(want_c, channel_counts)
    np.testing.assert_array_equal(want_b, baseline_counts)
