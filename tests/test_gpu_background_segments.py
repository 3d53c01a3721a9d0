"""The standalone background kernel (csrc/background.hip) where its two medians meet.

``background_kernel<WIDTH>`` computes a segment of channels per wavefront. For WIDTH <= 13 and
no input flags, a segment whose halo lies inside the band takes the merging median
(median_merge.h) in blocks of WIDTH channels, and is redone with the sorted window
(median_window.h) if any sample it read was NaN or infinite; the first and the last segment,
flagged input and widths 15 .. 31 take the sorted window from the start. The tests here walk
the segment length, the length of the last segment and the place of a single non-finite sample
through every value that changes what a wavefront does (tests/test_background_segments.py
states, from the launcher's own geometry, what each sweep covers), and every width 3 .. 31
through every flags mode and input kind.

Every comparison is exact against oracle.BackgroundMedianFilterHost rounded to float32 (the
sign of a zero aside: which of two equal zeros is the median is not defined by the host
either). The launches go through the C-ABI directly: one upload serves every band length of a
sweep, because the first `channels` rows of a [C][B] array are a band of their own.
"""

import ctypes

import numpy as np
import pytest

from katsdpsigproc_amd import _lib
from tests import inputs, inputs_background as ib

pytestmark = pytest.mark.gpu

MODE_VALUES = {"NONE": 0, "CHANNEL": 1, "FULL": 2}


class Gpu:
    def __init__(self):
        from katsdpsigproc_amd import accel

        self.context = accel.create_some_context(interactive=False)
        self.queue = self.context.create_command_queue()
        self.device = self.context.device.index
        self.stream = ctypes.c_void_p(self.queue.stream)

    def upload(self, host):
        from katsdpsigproc_amd import accel

        array = accel.DeviceArray(self.context, host.shape, host.dtype)
        array.set(self.queue, host)
        return array

    def empty(self, shape, dtype):
        from katsdpsigproc_amd import accel

        return accel.DeviceArray(self.context, shape, dtype)

    def background(self, d_in, d_out, d_flags, channels, width, mode, csplit):
        """The deviations of the first `channels` rows of d_in (complex64 or float32, rows of
        d_in.shape[1] baselines, no padding). d_out is filled with NaN first, and whatever lies
        behind the band must still be NaN afterwards."""
        rows, baselines = d_in.shape
        assert d_out.shape == d_in.shape and 0 < channels <= rows
        assert d_in.padded_shape == d_in.shape and d_out.padded_shape == d_out.shape
        flags_ptr, flags_stride = None, 0
        if mode != "NONE":
            want_shape = (rows,) if mode == "CHANNEL" else (rows, baselines)
            assert d_flags.shape == d_flags.padded_shape == want_shape
            flags_ptr = ctypes.c_void_p(d_flags.buffer.ptr)
            flags_stride = baselines if mode == "FULL" else 0
        _lib.call("ksp_memset_async", self.device, ctypes.c_void_p(d_out.buffer.ptr), 0xFF,
                  d_out.buffer.nbytes, self.stream)  # fmt: skip
        _lib.call("ksp_background_median_filter", self.device, self.stream,
                  ctypes.c_void_p(d_in.buffer.ptr), ctypes.c_void_p(d_out.buffer.ptr), flags_ptr,
                  channels, baselines, baselines, flags_stride, width,
                  int(d_in.dtype == np.float32), MODE_VALUES[mode], csplit)  # fmt: skip
        out = np.asarray(d_out.get(self.queue))
        assert np.isnan(out[channels:]).all(), "rows behind the band were written"
        return out[:channels]


@pytest.fixture(scope="module")
def gpu():
    return Gpu()


@pytest.fixture(scope="module")
def oracle():
    from oracle import rfi_oracle

    rfi_oracle.set_threads(min(rfi_oracle.max_threads(), 16))
    yield rfi_oracle
    rfi_oracle.set_threads(1)


def expected(oracle, width, data, flags=None):
    with np.errstate(over="ignore"):
        want = oracle.BackgroundMedianFilterHost(width, data.dtype == np.float32)(data, flags)
        return want.astype(np.float32)


def check(want, out, width, csplit, what):
    """Exact equality; a failure names the first wrong sample and the segment that wrote it."""
    if np.array_equal(want, out):
        return
    channels, baselines = want.shape
    with np.errstate(invalid="ignore"):
        wrong = np.argwhere(~(want == out))
    c, b = (int(v) for v in wrong[0])
    seg_len, n_segs = ib.geometry(channels, baselines, width, csplit)
    c_begin = c // seg_len * seg_len
    c_end = min(channels, c_begin + seg_len)
    where = (f"{what}: {len(wrong)} wrong, first at channel {c}, baseline {b}: segment "
             f"{c // seg_len} of {n_segs} = [{c_begin}, {c_end}), "
             f"{'merging' if ib.segment_merges(channels, width, c_begin, c_end) else 'sorted'} "
             f"unless flagged or non-finite, block {(c - c_begin) // width}, channel "
             f"{c - c_begin} of the segment")  # fmt: skip
    np.testing.assert_array_equal(want, out, err_msg=where)


# -------------------------------------------------------------------------- a. seam sweep
@pytest.mark.parametrize("kind", ["cplx", "amp"])
@pytest.mark.parametrize("width", ib.MERGE_WIDTHS)
def test_seams(width, kind, gpu, oracle):
    """No flags, 65 baselines (a full and a ragged wave column), every band length of
    inputs_background.seam_sweep: every residue of the segment length modulo the width in a
    merging segment (the partial last block and the clamped prefetch), every length of the
    last segment from 1 to width + 1 channels, the segment before it merging and not."""
    sweep = ib.seam_sweep(width)
    band = ib.make_band(ib.seam_sweep_max_channels(width), ib.SWEEP_BASELINES, kind, seed=width)
    d_in, d_out = gpu.upload(band), gpu.empty(band.shape, np.float32)
    merging = 0
    for csplit, channels in sweep:
        segs = ib.segments(channels, *ib.geometry(channels, ib.SWEEP_BASELINES, width, csplit))
        merging += sum(ib.segment_merges(channels, width, *seg) for seg in segs)
        out = gpu.background(d_in, d_out, None, channels, width, "NONE", csplit)
        check(expected(oracle, width, band[:channels]), out, width, csplit,
              f"width {width}, {kind}, {channels} channels, csplit {csplit}")  # fmt: skip
    assert merging >= len(sweep)


# ---------------------------------------------------------------------- b. fallback sweep
@pytest.mark.parametrize("kind", ["cplx", "amp"])
@pytest.mark.parametrize("width", ib.MERGE_WIDTHS)
def test_single_nonfinite_sample(width, kind, gpu, oracle):
    """One NaN or infinite sample per wave column, at channel k in wave column k: a wavefront
    is a wave column times a segment, so one launch puts the only bad sample of a wavefront at
    every place a merging segment reads -- its core, both halos, the first and the last sample
    -- and at every place it does not. The segment must notice it wherever it is."""
    channels, baselines, csplit = ib.fallback_shape(width)
    clean = ib.make_noise(channels, baselines, kind, seed=100 + width)
    rows, cols = ib.plant_positions(channels)
    d_in, d_out = gpu.empty(clean.shape, clean.dtype), gpu.empty(clean.shape, np.float32)
    for value in ib.nonfinite_values(kind):
        band = ib.plant(clean.copy(), rows, cols, value)
        d_in.set(gpu.queue, band)
        out = gpu.background(d_in, d_out, None, channels, width, "NONE", csplit)
        check(expected(oracle, width, band), out, width, csplit,
              f"width {width}, {kind}, one {value} per wave column")  # fmt: skip
        if np.isinf(value):
            assert np.array_equal(out[rows, cols], np.full(channels, value, np.float32))


# ---------------------------------------------------- c. every width, mode and input kind
@pytest.mark.parametrize("kind", ["cplx", "amp"])
@pytest.mark.parametrize("width", ib.ALL_WIDTHS)
def test_every_width_and_mode(width, kind, gpu, oracle):
    """Widths 3 .. 31 in every flags mode: three segments of 4 * width channels and a tail of
    1 .. 4 * width channels, then bands of 1 .. width + 1 channels (shorter than a window, or
    just not). With flags, and from width 15 on, every segment takes the sorted window."""
    long_bands, short_bands = ib.sorted_window_channels(width)
    rows = max(long_bands)
    band = ib.make_band(rows, ib.SWEEP_BASELINES, kind, seed=200 + width)
    chan, full = ib.make_masks(rows, ib.SWEEP_BASELINES, width, seed=300 + width)
    d_in, d_out = gpu.upload(band), gpu.empty(band.shape, np.float32)
    d_flags = {"NONE": None, "CHANNEL": gpu.upload(chan), "FULL": gpu.upload(full)}
    for modes, bands in ((ib.MODES, long_bands), (("NONE", "FULL"), short_bands)):
        for mode in modes:
            for channels in bands:
                flags = ib.mode_flags(mode, chan, full, channels)
                out = gpu.background(d_in, d_out, d_flags[mode], channels, width, mode, 3)
                check(expected(oracle, width, band[:channels], flags), out, width, 3,
                      f"width {width}, {kind}, {mode}, {channels} channels")  # fmt: skip


# ------------------------------------- d. the two broad tests of test_gpu_ops, without flags
def host_from_device(gpu, width, tuning=None):
    from katsdpsigproc_amd.rfi import device

    template = device.BackgroundMedianFilterDeviceTemplate(
        gpu.context, width, False, device.BackgroundFlags.NONE,
        **({} if tuning is None else {"tuning": tuning}),
    )  # fmt: skip
    return device.BackgroundHostFromDevice(template, gpu.queue)


@pytest.mark.parametrize("width", ib.ALL_WIDTHS)
def test_every_width_no_flags(width, gpu, oracle):
    """TestBackground.test_every_width of test_gpu_ops.py without input flags, so that widths
    up to 13 run the merging median in the interior segments (the tuned csplit of the
    template, 417 x 313)."""
    vis, _ = inputs.background_case()
    out = host_from_device(gpu, width)(vis)
    np.testing.assert_array_equal(expected(oracle, width, vis), out)


@pytest.mark.parametrize("csplit", [0, 1, 3, 8, 64, 1000])
def test_every_channel_split_no_flags(csplit, gpu, oracle):
    """TestBackground.test_every_channel_split of test_gpu_ops.py without input flags: the
    tunable only changes who computes what, and with which median; any split gives the same
    bits."""
    vis, _ = inputs.background_case()
    out = host_from_device(gpu, 13, {"wgs": 64, "csplit": csplit})(vis)
    check(expected(oracle, 13, vis), out, 13, csplit, f"csplit {csplit}")
