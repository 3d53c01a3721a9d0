"""Every launcher of the C-ABI on sub-views: raw pointers into larger allocations, a row stride
of its own per array, pointers that are not 16-byte aligned.

The launchers choose between 16-byte vector accesses and element-wise ones from the alignment
of their pointers and strides; through ``accel`` (rows padded to 128 bytes, pointers straight
from the allocator) only the vector side is ever chosen for rows of any length. Here every
array of a call is a :class:`tests.subviews.DeviceView`: inputs lie in poison (NaN, 0xFF),
outputs in sentinel bytes, and after each call every allocation is read back whole -- nothing
outside ``[row * stride, row * stride + cols)`` of a row may have changed, and no input at all.
Results are held to what the launcher's own test in test_gpu_ops.py / test_gpu_flagger.py
holds them to: bit-exact against ``oracle.rfi_oracle`` or NumPy, and maskedsum within
``1e-6 * sum(|x| * mask)``, the reference's own bound.

The alignment cases, as far as a signature allows them (V = elements per 16 bytes):
  A  everything 16-byte aligned: the vector path, as a control
  B  strides that are no multiple of V, pointers aligned
  C  aligned strides, the input pointer one element in
  D  aligned strides, the output pointer one element in
  E  B and C together
"""

import ctypes

import numpy as np
import pytest

from katsdpsigproc_amd import _lib
from tests import inputs, subviews

pytestmark = pytest.mark.gpu

F32 = np.float32


def up(n, multiple):
    return -(-n // multiple) * multiple


def row_stride(cols, odd, which=0):
    """A stride for rows of `cols` elements: a multiple of 16 elements (rows then start on
    multiples of 16 bytes whatever the type), or an odd number; `which` tells the arrays of a
    call apart, so that each has a stride of its own."""
    return up(cols, 16) + 16 * which + ((1 + 2 * which) if odd else 0)


#           odd strides, input offset, output offset
CASES = {"A": (False, 0, 0), "B": (True, 0, 0), "C": (False, 1, 0), "D": (False, 0, 1),
         "E": (True, 1, 0)}  # fmt: skip


def cases(names):
    return [(name,) + CASES[name] for name in names]


class Gpu:
    def __init__(self, context, queue):
        self.context, self.queue = context, queue
        self.device = context.device.index
        self.stream = ctypes.c_void_p(queue.stream)

    def input(self, data, stride=None, offset=0, role=None):
        """`data` (1-D: a single row) in poison; read() checks that it was left alone. `role`
        names the argument of the launcher that the view becomes."""
        data = np.atleast_2d(data)
        stride = data.shape[1] if stride is None else stride
        return self.view(data.dtype, data, stride, offset, True, role)

    def output(self, shape, dtype, stride=None, offset=0, role=None):
        """An array of sentinels among sentinels; read() checks everything around the rows."""
        shape = (1, shape) if np.isscalar(shape) else tuple(shape)
        stride = shape[1] if stride is None else stride
        blank = subviews.sentinel_array(shape, dtype)
        return self.view(dtype, blank, stride, offset, False, role)

    def view(self, dtype, data, stride, offset, poison, role):
        """The view factory: compact sub-views here, whatever the role. The bodies below take
        the strides they hand to a launcher from the views (or from :meth:`shared_stride`), so
        that another factory (tests/test_gpu_far_rows.py) may choose other strides."""
        return subviews.DeviceView(self.context, self.queue, dtype, data, stride, offset, poison)

    def shared_stride(self, like, arrays):
        """The one stride of `arrays`, (role, rows, cols, dtype) each, that a launcher takes
        for several arrays at once: `like`, the compact stride, here."""
        return like

    def call(self, name, *args):
        return _lib.call(name, self.device, self.stream, *args)


@pytest.fixture(scope="module")
def gpu():
    from katsdpsigproc_amd import accel

    context = accel.create_some_context(interactive=False)
    return Gpu(context, context.create_command_queue())


@pytest.fixture(scope="module")
def oracle():
    from oracle import rfi_oracle

    return rfi_oracle


def assert_equal(want, got, what):
    """Exact: float32 results as numpy compares them (a NaN only where the reference has one),
    which is what the launchers' own tests ask; anything else byte for byte."""
    want, got = np.ascontiguousarray(want), np.ascontiguousarray(got)
    assert want.dtype == got.dtype and want.shape == got.shape, what
    if want.dtype.kind == "f":
        np.testing.assert_array_equal(want, got, err_msg=what)
    else:
        np.testing.assert_array_equal(want.view(np.uint8), got.view(np.uint8), err_msg=what)


# ------------------------------------------------------------------------------ transpose
ELEMENT_TYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64, 16: np.complex128}
# one tile, ragged tiles in both directions, single rows and columns, a ragged corner
TRANSPOSE_SHAPES = [(64, 64), (65, 130), (130, 65), (1, 300), (300, 1), (67, 129)]
# (name, odd strides, src offset, dst offset): E once with the offset on either side
TRANSPOSE_CASES = cases("ABCD") + [("E-src", True, 1, 0), ("E-dst", True, 0, 1)]


@pytest.mark.parametrize("elem_size", sorted(ELEMENT_TYPES))
def test_transpose(elem_size, gpu):
    """1-, 2- and 4-byte elements move 4 per lane and 8-byte elements 2 when both pointers and
    both strides allow it; 16-byte elements always move singly (sub-view checks only)."""
    dtype = np.dtype(ELEMENT_TYPES[elem_size])
    rs = np.random.RandomState(elem_size)
    for rows, cols in TRANSPOSE_SHAPES:
        data = rs.randint(0, 256, (rows, cols * elem_size)).astype(np.uint8).view(dtype)
        want = np.ascontiguousarray(data.T)
        for name, odd, src_offset, dst_offset in TRANSPOSE_CASES:
            what = f"{rows} x {cols} x {elem_size} B, case {name}"
            run_transpose(gpu, data, want, odd, src_offset, dst_offset, what)


def run_transpose(gpu, data, want, odd, src_offset, dst_offset, what):
    rows, cols = data.shape
    src = gpu.input(data, row_stride(cols, odd), src_offset, role="in")
    dst = gpu.output((cols, rows), data.dtype, row_stride(rows, odd, 1), dst_offset, role="out")
    gpu.call("ksp_transpose", dst.ptr, src.ptr, rows, cols, dst.stride, src.stride,
             data.dtype.itemsize)  # fmt: skip
    assert_equal(want, dst.read("dst, " + what), what)
    src.read("src, " + what)


# ----------------------------------------------------------------------------- percentile5
P5_COLUMNS = [100, 1024, 1025, 1100, 4096, 4097]  # workgroup | wavefront (1025..4096) | workgroup
P5_LONG_COLUMNS = [16385, 20000]  # radix select


def p5_signed(n_cols):
    """The wavefront and the radix-select kernels are exact for signed values; the workgroup
    kernel of the other widths is the reference's search, for positive values."""
    return 1024 < n_cols <= 4096 or n_cols > 16384


def p5_case(rs, oracle, rows, n_cols, is_amplitude):
    if is_amplitude:
        data = rs.standard_normal((rows, n_cols)).astype(F32)
        data[:, ::7] = 0.25  # ties
        data[:, 3::7] = -0.5
        if not p5_signed(n_cols):
            data = np.abs(data)
        want = np.percentile(data, [0, 100, 25, 75, 50], axis=1, method="lower").astype(F32)
    else:
        data = inputs.complex_normal(rs, size=(rows, n_cols)).astype(np.complex64)
        want = oracle.percentile5(data)
    return data, want


def p5_run(gpu, data, want, first_col, in_stride, in_offset, is_amplitude, what):
    rows, n_cols = data.shape
    # the rows of the call start first_col elements in front of the data: those columns, like
    # the ones behind the range, are poison
    src = gpu.input(data, in_stride, in_offset + first_col, role="in")
    base = ctypes.c_void_p(src.address - first_col * data.dtype.itemsize)
    out = gpu.output((5, rows), F32, rows + 3, role="out")
    gpu.call("ksp_percentile5_float", base, out.ptr, rows, src.stride, out.stride, first_col,
             n_cols, int(is_amplitude))  # fmt: skip
    assert_equal(want, out.read("out, " + what), what)
    src.read("in, " + what)


def p5_layouts(n_cols, first_cols):
    """(first_col, in_stride, in_offset): strides that are a multiple of 4 (16-byte loads of
    float32 and of complex64 where first_col and the pointer allow them), odd, and even but no
    multiple of 4 (16-byte loads of complex64 only); the pointer aligned or one element in."""
    for first_col in first_cols:
        base = up(first_col + n_cols, 4) + 4
        for in_stride in (base, base + 1, base + 2):
            for in_offset in (0, 1):
                yield first_col, in_stride, in_offset


@pytest.mark.parametrize("rows", [1, 4, 5])  # a workgroup of the wavefront kernel holds 4 rows
@pytest.mark.parametrize("is_amplitude", [True, False])
def test_percentile5(is_amplitude, rows, gpu, oracle):
    rs = np.random.RandomState(rows)
    for n_cols in P5_COLUMNS:
        data, want = p5_case(rs, oracle, rows, n_cols, is_amplitude)
        for first_col, in_stride, in_offset in p5_layouts(n_cols, (0, 1, 2, 3, 4)):
            what = (f"{rows} x {n_cols}, first_col {first_col}, stride {in_stride}, "
                    f"offset {in_offset}, amplitude {is_amplitude}")  # fmt: skip
            p5_run(gpu, data, want, first_col, in_stride, in_offset, is_amplitude, what)


@pytest.mark.parametrize("is_amplitude", [True, False])
def test_percentile5_long(is_amplitude, gpu, oracle):
    rs = np.random.RandomState(7)
    for n_cols in P5_LONG_COLUMNS:
        data, want = p5_case(rs, oracle, 3, n_cols, is_amplitude)
        for first_col, in_stride, in_offset in p5_layouts(n_cols, (0, 1, 3)):
            what = (f"3 x {n_cols}, first_col {first_col}, stride {in_stride}, "
                    f"offset {in_offset}, amplitude {is_amplitude}")  # fmt: skip
            p5_run(gpu, data, want, first_col, in_stride, in_offset, is_amplitude, what)


# --------------------------------------------------------------------------------- madnz
def madl_stage_max():
    """MADL_STAGE_MAX of csrc/madnz_long.h: rows of up to so many channels are staged in LDS,
    longer ones are streamed."""
    import os
    import re

    from katsdpsigproc_amd import build_native

    with open(os.path.join(build_native.CSRC, "madnz_long.h")) as f:
        return int(re.search(r"#define MADL_STAGE_MAX (\d+)", f.read()).group(1))


MADL_STAGE_MAX = madl_stage_max()
MADT_CHANNELS = [100, 1024, 1025, 1100, 4096, 4097, MADL_STAGE_MAX, MADL_STAGE_MAX + 1]


def noise_case(rs, oracle, channels, baselines):
    """(deviations [C][B] with a tenth of exact zeros, which the median leaves out; the oracle's
    noise as float32)."""
    dev = rs.standard_normal((channels, baselines)).astype(F32)
    dev[rs.random_sample(dev.shape) < 0.1] = 0.0
    dev[:, 0][rs.random_sample(channels) < 0.5] = -0.0  # one baseline half zeros, of either sign
    assert (dev == 0).any() or dev.size < 10
    return dev, oracle.NoiseEstMADHost()(dev).astype(F32)


@pytest.mark.parametrize("baselines", [1, 4, 5])  # a workgroup of the wavefront kernel holds 4
def test_madnz_t(baselines, gpu, oracle):
    rs = np.random.RandomState(baselines)
    for channels in MADT_CHANNELS:
        dev, want = noise_case(rs, oracle, channels, baselines)
        data = np.ascontiguousarray(dev.T)
        for name, odd, in_offset, _ in cases("ABCE"):
            what = f"{channels} channels, {baselines} baselines, case {name}"
            run_madnz(gpu, "ksp_madnz_t", data, want, row_stride(channels, odd), in_offset,
                      int(name != "A"), what)  # fmt: skip


def run_madnz(gpu, launcher, data, want, stride, in_offset, out_offset, what):
    """ksp_madnz_t on data [B][stride], ksp_madnz on data [C][stride]."""
    channels, baselines = data.shape[::-1] if launcher == "ksp_madnz_t" else data.shape
    src = gpu.input(data, stride, in_offset, role="in")
    noise = gpu.output(baselines, F32, offset=out_offset)
    gpu.call(launcher, src.ptr, noise.ptr, channels, baselines, src.stride)
    assert_equal(want[np.newaxis], noise.read("noise, " + what), what)
    src.read("in, " + what)


# the strip kernel (up to 4096 channels): 8 baselines per workgroup, loaded four at a time
# with one 16-byte load where four are left; more channels: 64 baselines per workgroup
MADNZ_SHAPES = [(c, b) for c in (100, 4096) for b in (1, 7, 8, 9, 12)] + [
    (4100, b) for b in (63, 64, 65)]  # fmt: skip


@pytest.mark.parametrize("channels, baselines", MADNZ_SHAPES)
def test_madnz(channels, baselines, gpu, oracle):
    rs = np.random.RandomState(channels + baselines)
    dev, want = noise_case(rs, oracle, channels, baselines)
    for name, odd, in_offset, _ in cases("ABCE"):
        what = f"{channels} channels, {baselines} baselines, case {name}"
        run_madnz(gpu, "ksp_madnz", dev, want, row_stride(baselines, odd), in_offset,
                  int(name != "A"), what)  # fmt: skip


# ---------------------------------------------------------------------- threshold_simple
SIMPLE_COLS = [1, 3, 4, 5, 1023, 1024, 1025, 1027]  # a lane owns 4 columns, a workgroup 1024


@pytest.mark.parametrize("transposed", [False, True])
def test_threshold_simple(transposed, gpu, oracle):
    """deviations and flags share one stride; the 16-byte loads need aligned deviations and the
    4-byte stores aligned flags, which is checked separately (case D moves the flags alone)."""
    rs = np.random.RandomState(int(transposed))
    flagged = total = 0
    for rows in (1, 3):
        for cols in SIMPLE_COLS:
            dev, noise, want = simple_case(rs, oracle, rows, cols, transposed)
            flagged += np.count_nonzero(want)
            total += want.size
            for name, odd, in_offset, out_offset in cases("ABCDE"):
                what = f"{rows} x {cols}, transposed {transposed}, case {name}"
                run_threshold_simple(gpu, dev, noise, want, transposed, row_stride(cols, odd),
                                     in_offset, out_offset, what)  # fmt: skip
    assert 0.4 < flagged / total < 0.6


SIMPLE_N_SIGMA, SIMPLE_FLAG_VALUE = 11.0, 4


def simple_case(rs, oracle, rows, cols, transposed):
    """(deviations, noise, the oracle's flags), the two arrays as the launcher takes them:
    [rows][cols], which is [B][C] if `transposed`."""
    n_sigma, flag_value = SIMPLE_N_SIGMA, SIMPLE_FLAG_VALUE
    channels, baselines = (cols, rows) if transposed else (rows, cols)
    noise = rs.uniform(5.0, 15.0, baselines).astype(F32)
    limit = np.broadcast_to(F32(n_sigma) * noise, (channels, baselines))  # float32 product
    # about half above the limit; some exactly on it (not flagged: the comparison is a
    # strict >) and some one float32 above it
    dev = (limit * rs.uniform(0.0, 2.0, limit.shape)).astype(F32)
    pick = rs.random_sample(limit.shape)
    exact, above = pick < 0.15, (pick >= 0.15) & (pick < 0.3)
    dev[exact] = limit[exact]
    dev[above] = np.nextafter(limit[above], F32(np.inf))
    want = oracle.ThresholdSimpleHost(n_sigma, flag_value)(dev, noise)
    assert not want[exact].any() and np.all(want[above] == flag_value)
    if transposed:
        dev, want = np.ascontiguousarray(dev.T), np.ascontiguousarray(want.T)
    return dev, noise, want


def shared(gpu, like, dev):
    """The stride that deviations (float32) and flags (uint8) of one shape share."""
    return gpu.shared_stride(like, [("deviations",) + dev.shape + (F32,),
                                    ("flags",) + dev.shape + (np.uint8,)])  # fmt: skip


def run_threshold_simple(gpu, dev, noise, want, transposed, stride, in_offset, out_offset, what):
    rows, cols = dev.shape
    stride = shared(gpu, stride, dev)
    d_dev = gpu.input(dev, stride, in_offset, role="deviations")
    d_noise = gpu.input(noise, offset=in_offset)
    d_flags = gpu.output((rows, cols), np.uint8, stride, out_offset, role="flags")
    gpu.call("ksp_threshold_simple", d_dev.ptr, d_noise.ptr, d_flags.ptr, rows, cols,
             stride, SIMPLE_N_SIGMA, SIMPLE_FLAG_VALUE, int(transposed))  # fmt: skip
    assert_equal(want, d_flags.read("flags, " + what), what)
    d_dev.read("deviations, " + what)
    d_noise.read("noise, " + what)


# ------------------------------------------------------------------------- threshold_sum
def sum_case(oracle, channels, baselines):
    """Deviations of inputs.add_rfi visibilities from their median background, and their noise
    (both float32, as the stages before the threshold leave them), with the oracle's flags."""
    vis = inputs.add_rfi(inputs.generate_data(channels, baselines, seed=channels), seed=baselines)
    dev = oracle.BackgroundMedianFilterHost(13)(vis).astype(F32)
    noise = oracle.NoiseEstMADHost()(dev).astype(F32)
    return dev, noise, oracle.ThresholdSumHost(11.0)(dev, noise)


@pytest.fixture(scope="module")
def sum_cases(oracle):
    return {(c, b): sum_case(oracle, c, b) for c in (9, 257, 2100) for b in (1, 5, 65)}


SUM_SCALES = (ctypes.c_float * 4)(*[F32(pow(1.2, -i)) for i in range(4)])


@pytest.mark.parametrize("channel_major", [False, True])
def test_threshold_sum(channel_major, gpu, sum_cases):
    """ksp_threshold_sum on [B][C] and ksp_threshold_sum_cm on [C][B]; deviations and flags
    share one stride."""
    flagged = 0
    for (channels, baselines), (dev, noise, want) in sum_cases.items():
        flagged += np.count_nonzero(want)
        if not channel_major:
            dev, want = np.ascontiguousarray(dev.T), np.ascontiguousarray(want.T)
        for name, odd, in_offset, out_offset in cases("ABCD"):
            what = f"{channels} x {baselines}, channel-major {channel_major}, case {name}"
            run_threshold_sum(gpu, dev, noise, want, channel_major, row_stride(dev.shape[1], odd),
                              in_offset, out_offset, what)  # fmt: skip
    assert flagged > 0


def run_threshold_sum(gpu, dev, noise, want, channel_major, stride, in_offset, out_offset, what):
    """`dev` and `want` as the launcher takes them: [C][B] if `channel_major`, else [B][C]."""
    channels, baselines = dev.shape if channel_major else dev.shape[::-1]
    stride = shared(gpu, stride, dev)
    d_dev = gpu.input(dev, stride, in_offset, role="deviations")
    d_noise = gpu.input(noise, offset=in_offset)
    d_flags = gpu.output(dev.shape, np.uint8, stride, out_offset, role="flags")
    if channel_major:
        gpu.call("ksp_threshold_sum_cm", d_dev.ptr, d_noise.ptr, d_flags.ptr, channels,
                 baselines, stride, 11.0, SUM_SCALES, 4, 1)  # fmt: skip
    else:
        gpu.call("ksp_threshold_sum", d_dev.ptr, d_noise.ptr, d_flags.ptr, channels,
                 baselines, stride, 11.0, SUM_SCALES, 4, 1, 0)  # fmt: skip
    assert_equal(want, d_flags.read("flags, " + what), what)
    d_dev.read("deviations, " + what)
    d_noise.read("noise, " + what)


# ---------------------------------------------------------------------------- background
@pytest.fixture(scope="module")
def background_inputs(oracle):
    """vis, |vis| and per-sample input flags for the largest shape; smaller ones are its
    top-left corner."""
    rs = np.random.RandomState(5)
    vis = inputs.complex_normal(rs, size=(700, 130)).astype(np.complex64)
    flags = np.where(rs.random_sample(vis.shape) < 0.1, rs.randint(1, 256, vis.shape), 0)
    flags = flags.astype(np.uint8)
    flags[100:125, 3:70] = 4  # whole windows without a sample
    return vis, oracle.abs_c64(vis), flags


@pytest.mark.parametrize("mode", ["NONE", "CHANNEL", "FULL"])
@pytest.mark.parametrize("width", [3, 13, 33])  # 33: the wide-window kernel
def test_background(width, mode, gpu, oracle, background_inputs):
    """in and out share `stride`; per-sample flags have a stride of their own."""
    for is_amplitude in (True, False):
        for channels in (40, 700):
            for baselines in (1, 63, 65, 130):
                data = background_inputs[1 if is_amplitude else 0][:channels, :baselines]
                flags = {"NONE": None, "CHANNEL": background_inputs[2][:channels, 0],
                         "FULL": background_inputs[2][:channels, :baselines]}[mode]  # fmt: skip
                want = oracle.BackgroundMedianFilterHost(width, is_amplitude)(data, flags).astype(F32)
                for name, odd, in_offset, _ in cases("ABC"):
                    what = (f"{channels} x {baselines}, width {width}, {mode}, amplitude "
                            f"{is_amplitude}, case {name}")  # fmt: skip
                    run_background(gpu, data, flags, want, width, mode, odd, in_offset, what)


def run_background(gpu, data, flags, want, width, mode, odd, in_offset, what):
    channels, baselines = data.shape
    is_amplitude = data.dtype == F32
    stride = gpu.shared_stride(row_stride(baselines, odd), [("in",) + data.shape + (data.dtype,),
                                                            ("out",) + data.shape + (F32,)])  # fmt: skip
    src = gpu.input(data, stride, in_offset, role="in")
    out = gpu.output((channels, baselines), F32, stride, role="out")
    d_flags, flags_stride = None, 0
    if mode == "CHANNEL":
        d_flags = gpu.input(flags, offset=in_offset)
    elif mode == "FULL":
        d_flags = gpu.input(flags, row_stride(baselines, odd, 1), in_offset, role="flags")
        flags_stride = d_flags.stride
    gpu.call("ksp_background_median_filter", src.ptr, out.ptr,
             None if d_flags is None else d_flags.ptr, channels, baselines, stride,
             flags_stride, width, int(is_amplitude), {"NONE": 0, "CHANNEL": 1, "FULL": 2}[mode],
             0)  # fmt: skip
    assert_equal(want, out.read("out, " + what), what)
    src.read("in, " + what)
    if d_flags is not None:
        d_flags.read("flags, " + what)


# ----------------------------------------------------------------------------- maskedsum
@pytest.mark.parametrize("use_amplitudes", [False, True])
def test_maskedsum(use_amplitudes, gpu, oracle):
    """A workgroup covers 16 columns and 64 row phases. `out` (one row) is one element into
    its allocation in every case but the control."""
    rs = np.random.RandomState(3)
    for rows, cols in [(37, 100), (130, 15), (130, 16), (130, 17)]:
        data = rs.randn(rows, cols, 2).astype(F32).view(np.complex64)[..., 0]
        mask = (rs.random_sample(rows) < 0.7).astype(F32)
        want = oracle.maskedsum(data, mask, use_amplitudes)
        scale = np.sum(np.abs(data) * mask[:, None], axis=0)  # cancellation-safe tolerance
        for name, odd, in_offset, _ in cases("ABC"):
            what = f"{rows} x {cols}, amplitudes {use_amplitudes}, case {name}"
            run_maskedsum(gpu, data, mask, want, scale, use_amplitudes, row_stride(cols, odd),
                          in_offset, int(name != "A"), what)  # fmt: skip


def run_maskedsum(gpu, data, mask, want, scale, use_amplitudes, stride, in_offset, out_offset, what):
    rows, cols = data.shape
    src = gpu.input(data, stride, in_offset, role="in")
    d_mask = gpu.input(mask, offset=in_offset)
    out = gpu.output(cols, F32 if use_amplitudes else np.complex64, offset=out_offset)
    gpu.call("ksp_maskedsum_float", src.ptr, d_mask.ptr, out.ptr, src.stride, rows, cols,
             int(use_amplitudes))  # fmt: skip
    got = out.read("out, " + what)[0]
    np.testing.assert_array_less(np.abs(got - want), 1e-6 * scale + 1e-30, err_msg=what)
    src.read("in, " + what)
    d_mask.read("mask, " + what)


# ------------------------------------------------------------------------- fused flagger
FUSED_SCALES = (ctypes.c_double * 4)(*[pow(1.2, -i) for i in range(4)])
STRIP, LONG, RING = _lib.FUSED_PATH_STRIP, _lib.FUSED_PATH_LONG, _lib.FUSED_PATH_RING
# (channels, baselines, width, deviations output, ring mode, kernels launched, which is ...)
FUSED_SHAPES = [
    pytest.param(200, 10, 13, True, 0, STRIP, id="lanes-of-4"),  # flagger_fused_kernel<4, 13>
    # rows wide enough for whole 16-byte pieces in the row-wise zero fill of flags, starting
    # at every alignment (the stride of 75 is odd)
    pytest.param(200, 70, 13, True, 0, STRIP, id="lanes-of-4-wide-rows"),
    pytest.param(1000, 10, 13, True, 0, STRIP, id="lanes-of-16"),  # <16, 13>
    pytest.param(4096, 12, 13, False, 1, RING | STRIP, id="ring"),  # ring + 4 baselines left over
    pytest.param(4096, 12, 13, True, 0, STRIP, id="lanes-of-64"),  # <64, 13>
    pytest.param(600, 10, 21, True, 0, STRIP, id="width-21"),
    pytest.param(8192, 6, 13, True, 0, LONG, id="long"),  # flagger_long_kernel
]


@pytest.mark.parametrize("channels, baselines, width, keep_deviations, ring, path", FUSED_SHAPES)
def test_flagger_fused(channels, baselines, width, keep_deviations, ring, path, gpu, oracle):
    """`vis` is 16-byte aligned with an even stride, as the ABI requires; every other array is
    a sub-view. `flags` in particular is a column block of a wider array: the zero fill ahead
    of the kernel may clear its rows and nothing between them."""
    vis, masks = fused_inputs(channels, baselines, width)
    for mode in ("NONE", "CHANNEL", "FULL"):
        if ring and mode != "NONE":
            continue  # the ring kernel takes no input flags
        run_flagger_fused(gpu, oracle, vis, masks[mode], mode, width, keep_deviations, ring, path)


def fused_inputs(channels, baselines, width):
    """(vis, input flags per mode) for a shape of FUSED_SHAPES."""
    vis = inputs.add_rfi(inputs.generate_data(channels, baselines, seed=width), seed=baselines)
    rs = np.random.RandomState(channels)
    masks = {"NONE": None, "CHANNEL": inputs.channel_mask(channels, seed=3) * np.uint8(2),
             "FULL": (rs.random_sample(vis.shape) < 1.0 / 16.0).astype(np.uint8) * np.uint8(2)}  # fmt: skip
    return vis, masks


def run_flagger_fused(gpu, oracle, vis, mask, mode, width, keep_deviations, ring, path):
    from katsdpsigproc_amd import accel

    channels, baselines = vis.shape
    what = f"{channels} x {baselines}, width {width}, {mode}"
    want_flags, want_noise, want_dev = oracle.flagger_full(
        vis, mask, width=width, n_sigma=11.0, want_deviations=True)
    assert want_flags.any(), what
    d_vis = gpu.input(vis, baselines + 2, role="vis")
    assert d_vis.address % 16 == 0 and d_vis.stride % 2 == 0
    d_mask, mask_stride = None, 0
    if mode == "CHANNEL":
        d_mask = gpu.input(mask, offset=1)
    elif mode == "FULL":
        d_mask = gpu.input(mask, baselines + 7, offset=1, role="in_flags")
        mask_stride = d_mask.stride
    d_flags = gpu.output(vis.shape, np.uint8, baselines + 5, role="flags")
    d_noise = gpu.output(baselines, F32, offset=1)
    d_dev = gpu.output(vis.shape, F32, baselines + 3, role="deviations") if keep_deviations else None
    workspace = accel.DeviceArray(gpu.context, (16,), np.uint32)  # 64 bytes, zeroed once
    workspace.zero(gpu.queue)
    with _lib.fused_ring_mode(ring):
        gpu.call("ksp_flagger_fused", d_vis.ptr, None if d_mask is None else d_mask.ptr,
                 d_flags.ptr, None if d_dev is None else d_dev.ptr, d_noise.ptr, channels,
                 baselines, d_vis.stride, mask_stride, d_flags.stride,
                 0 if d_dev is None else d_dev.stride, width, 0,
                 {"NONE": 0, "CHANNEL": 1, "FULL": 2}[mode], 1, 11.0,
                 FUSED_SCALES, 4, 1, ctypes.c_void_p(workspace.buffer.ptr))  # fmt: skip
        assert _lib.call("ksp_flagger_fused_last_path") == path, what
    assert_equal(want_flags, d_flags.read("flags, " + what), what)
    assert_equal(want_noise.astype(F32)[np.newaxis], d_noise.read("noise, " + what), what)
    if d_dev is not None:
        assert_equal(want_dev.astype(F32), d_dev.read("deviations, " + what), what)
    d_vis.read("vis, " + what)
    if d_mask is not None:
        d_mask.read("in_flags, " + what)
    assert not workspace.get(gpu.queue).any(), "the workspace was not left zeroed: " + what
