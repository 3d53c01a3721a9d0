"""Every launcher of the C-ABI that takes a pointer and a row stride, on rows that lie more
than 2**31 and 2**32 bytes behind that pointer (tests/farviews.py has the layout and what it
guarantees).

The call bodies are those of the compact sub-view tests (tests/test_gpu_subviews.py and the
raw-ABI tests of the per-operation modules), run with another view factory: the arrays named in
`far` get a far stride of the same alignment class as their compact one and lie in one arena
that the module shares, every other array stays compact. The references and the bars are the
bodies' own: ``oracle.rfi_oracle``, ``rfi.host`` or NumPy, bit for bit, and maskedsum within the
reference's bound; never a compact run of the same kernel.

Each strided argument is far once on its own and once together with the others. Arrays that
share one stride argument (deviations and flags of the threshold launchers, in and out of the
background filter) can only move together: each takes a turn at choosing the stride, so that the
narrower type's rows, too, cross 2**32 bytes (the wider one's then span four or eight times as
much). Arrays without a row stride stay compact. Where one arena cannot hold every array of a
launcher at once (seven or more arrays of 6 GiB), the inputs, the outputs and the accumulators
are far together instead. Both stride classes of the compact tests take part wherever the body
has both: rows on 16-byte boundaries, and odd strides (even ones that are no multiple of 16 for
`vis`); the bodies of average, solve_gains and fit_delays know odd strides only.

Device memory: one arena of 31 GiB for the module (the `arena` fixture checks its use).
"""

import ctypes

import numpy as np
import pytest

from katsdpsigproc_amd import _lib
from tests import farviews, inputs, subviews
from tests import test_gpu_subviews as sv

pytestmark = pytest.mark.gpu

F32, C64, U8 = np.float32, np.complex64, np.uint8
DEVICE_CAP = 32 << 30  # no test may hold more device memory at once
ARENA_BYTES = 31 << 30  # the whole module's far device memory


class FarGpu(sv.Gpu):
    """test_gpu_subviews.Gpu with the arrays of the roles `far` far."""

    def __init__(self, gpu, arena, far):
        super().__init__(gpu.context, gpu.queue)
        self.views = farviews.FarViews(arena, far, subviews.CompactViews(gpu.context, gpu.queue))
        self.shared_stride, self.check = self.views.shared_stride, self.views.check

    def view(self, dtype, data, stride, offset, poison, role):
        return self.views(role, dtype, data, stride, offset, poison)[0]


@pytest.fixture(scope="module")
def gpu():
    from katsdpsigproc_amd import accel

    context = accel.create_some_context(interactive=False)
    return sv.Gpu(context, context.create_command_queue())


@pytest.fixture(scope="module")
def arena(gpu):
    """The module's far device memory, all of it; what the compact arrays beside it take is
    kilobytes. The most that any test took of it is checked at the end."""
    arena = farviews.Arena(gpu.context, gpu.queue, ARENA_BYTES)
    yield arena
    assert 0 < arena.peak <= arena.n_bytes <= DEVICE_CAP - (512 << 20)


@pytest.fixture(scope="module")
def oracle():
    from oracle import rfi_oracle

    return rfi_oracle


def turns(*roles):
    """Each role far on its own, then all of them."""
    each = [(role,) for role in roles]
    return each + ([tuple(roles)] if len(roles) > 1 else [])


def ids(far):
    return "+".join(far)


ODD = [pytest.param(False, id="aligned"), pytest.param(True, id="odd")]


# ------------------------------------------------------------------------------ transpose
@pytest.mark.parametrize("far", turns("in", "out"), ids=ids)
@pytest.mark.parametrize("odd", ODD)
@pytest.mark.parametrize("elem_size", sorted(sv.ELEMENT_TYPES))
def test_transpose(elem_size, odd, far, gpu, arena):
    """67 x 129: ragged tiles both ways; the source has 67 far rows, the destination 129."""
    dtype = np.dtype(sv.ELEMENT_TYPES[elem_size])
    rows, cols = 67, 129
    data = np.random.RandomState(elem_size).randint(0, 256, (rows, cols * elem_size))
    data = data.astype(U8).view(dtype)
    fg = FarGpu(gpu, arena, far)
    sv.run_transpose(fg, data, np.ascontiguousarray(data.T), odd, 0, 0, f"far {far}")
    fg.check()


# ----------------------------------------------------------------------------- percentile5
@pytest.mark.parametrize("far", turns("in", "out"), ids=ids)
@pytest.mark.parametrize("is_amplitude", [True, False])
@pytest.mark.parametrize("n_cols", [100, 1100, 16385])  # workgroup, wavefront, radix select
def test_percentile5(n_cols, is_amplitude, far, gpu, arena, oracle):
    """5 rows (a workgroup of the wavefront kernel holds 4); `out` is (5, rows), so its far
    axis has the five percentiles. Strides: aligned, odd, and even but no multiple of 4."""
    rows = 5
    data, want = sv.p5_case(np.random.RandomState(n_cols), oracle, rows, n_cols, is_amplitude)
    base = sv.up(1 + n_cols, 4) + 4
    for in_stride in (base, base + 1, base + 2):
        fg = FarGpu(gpu, arena, far)
        sv.p5_run(fg, data, want, 1, in_stride, 0, is_amplitude, f"far {far}, like {in_stride}")
        fg.check()


# ---------------------------------------------------------------------------------- madnz
@pytest.mark.parametrize("odd", ODD)
@pytest.mark.parametrize("channels", [1100, 4097, sv.MADL_STAGE_MAX + 1])
def test_madnz_t(channels, odd, gpu, arena, oracle):
    """in: [B][stride] with 5 baselines far apart; wavefront, staged and streaming kernels."""
    dev, want = sv.noise_case(np.random.RandomState(channels), oracle, channels, 5)
    fg = FarGpu(gpu, arena, {"in"})
    sv.run_madnz(fg, "ksp_madnz_t", np.ascontiguousarray(dev.T), want,
                 sv.row_stride(channels, odd), 0, 1, f"{channels} channels")  # fmt: skip
    fg.check()


@pytest.mark.parametrize("odd", ODD)
@pytest.mark.parametrize("channels, baselines", [(100, 9), (4096, 12), (4100, 65)])
def test_madnz(channels, baselines, odd, gpu, arena, oracle):
    """in: [C][stride], the channels far apart; the strip kernel and the one for long bands."""
    dev, want = sv.noise_case(np.random.RandomState(channels), oracle, channels, baselines)
    fg = FarGpu(gpu, arena, {"in"})
    sv.run_madnz(fg, "ksp_madnz", dev, want, sv.row_stride(baselines, odd), 0, 1,
                 f"{channels} x {baselines}")  # fmt: skip
    fg.check()


# ------------------------------------------------------------------------------ thresholds
@pytest.mark.parametrize("far", turns("deviations", "flags"), ids=ids)
@pytest.mark.parametrize("odd", ODD)
@pytest.mark.parametrize("transposed", [False, True])
def test_threshold_simple(transposed, odd, far, gpu, arena, oracle):
    rs = np.random.RandomState(int(transposed))
    for rows, cols in [(3, 5), (3, 1027)]:
        dev, noise, want = sv.simple_case(rs, oracle, rows, cols, transposed)
        assert want.any()
        fg = FarGpu(gpu, arena, far)
        sv.run_threshold_simple(fg, dev, noise, want, transposed, sv.row_stride(cols, odd), 0, 0,
                                f"{rows} x {cols}, far {far}")  # fmt: skip
        fg.check()


@pytest.fixture(scope="module")
def sum_cases(oracle):
    return {(c, b): sv.sum_case(oracle, c, b) for c, b in [(257, 5), (2100, 65)]}


@pytest.mark.parametrize("far", turns("deviations", "flags"), ids=ids)
@pytest.mark.parametrize("odd", ODD)
@pytest.mark.parametrize("shape", [(257, 5), (2100, 65)], ids=str)
@pytest.mark.parametrize("channel_major", [False, True])
def test_threshold_sum(channel_major, shape, odd, far, gpu, arena, sum_cases):
    """ksp_threshold_sum on [B][C] (5 or 65 far rows) and ksp_threshold_sum_cm on [C][B]."""
    dev, noise, want = sum_cases[shape]
    assert want.any()
    if not channel_major:
        dev, want = np.ascontiguousarray(dev.T), np.ascontiguousarray(want.T)
    fg = FarGpu(gpu, arena, far)
    sv.run_threshold_sum(fg, dev, noise, want, channel_major, sv.row_stride(dev.shape[1], odd),
                         0, 0, f"{shape}, far {far}")  # fmt: skip
    fg.check()


# ---------------------------------------------------------------------------- background
@pytest.fixture(scope="module")
def background_inputs(oracle):
    rs = np.random.RandomState(5)
    vis = inputs.complex_normal(rs, size=(700, 65)).astype(C64)
    flags = np.where(rs.random_sample(vis.shape) < 0.1, rs.randint(1, 256, vis.shape), 0)
    flags = flags.astype(U8)
    flags[100:125, 3:60] = 4  # whole windows without a sample
    return vis, oracle.abs_c64(vis), flags


@pytest.mark.parametrize("far", turns("in", "out", "flags"), ids=ids)
@pytest.mark.parametrize("odd", ODD)
@pytest.mark.parametrize("is_amplitude", [True, False])
@pytest.mark.parametrize("width, channels", [(3, 40), (13, 700), (33, 700)])  # 33: the wide kernel
def test_background(width, channels, is_amplitude, odd, far, gpu, arena, oracle, background_inputs):
    """in and out share `stride` ("in" far: the stride is chosen for the input's type, "out"
    far: for float32); per-sample flags have a stride of their own."""
    data = background_inputs[1 if is_amplitude else 0][:channels]
    flags = background_inputs[2][:channels]
    want = oracle.BackgroundMedianFilterHost(width, is_amplitude)(data, flags).astype(F32)
    fg = FarGpu(gpu, arena, far)
    sv.run_background(fg, data, flags, want, width, "FULL", odd, 0, f"width {width}, far {far}")
    fg.check()


# ----------------------------------------------------------------------------- maskedsum
@pytest.mark.parametrize("odd", ODD)
@pytest.mark.parametrize("use_amplitudes", [False, True])
@pytest.mark.parametrize("rows, cols", [(37, 100), (130, 17)])
def test_maskedsum(rows, cols, use_amplitudes, odd, gpu, arena, oracle):
    rs = np.random.RandomState(3)
    data = rs.randn(rows, cols, 2).astype(F32).view(C64)[..., 0]
    mask = (rs.random_sample(rows) < 0.7).astype(F32)
    want = oracle.maskedsum(data, mask, use_amplitudes)
    scale = np.sum(np.abs(data) * mask[:, None], axis=0)  # the reference's own bound
    fg = FarGpu(gpu, arena, {"in"})
    sv.run_maskedsum(fg, data, mask, want, scale, use_amplitudes, sv.row_stride(cols, odd), 0, 1,
                     f"{rows} x {cols}")  # fmt: skip
    fg.check()


# ------------------------------------------------------------------------- fused flagger
# (channels, baselines): the strip kernel with lanes of 4, 16 and 64 channels, the kernel for
# long bands
FUSED_SHAPES = [pytest.param(256, 10, id="lanes-of-4"), pytest.param(1024, 10, id="lanes-of-16"),
                pytest.param(4096, 12, id="lanes-of-64"), pytest.param(8192, 6, id="long")]  # fmt: skip


@pytest.mark.parametrize("far", turns("vis", "in_flags", "flags", "deviations"), ids=ids)
@pytest.mark.parametrize("channels, baselines", FUSED_SHAPES)
def test_flagger_fused(channels, baselines, far, gpu, arena, oracle):
    """Per-sample input flags (mode FULL) and the deviations output, so that all four strided
    arrays take part."""
    vis, masks = sv.fused_inputs(channels, baselines, 13)
    fg = FarGpu(gpu, arena, far)
    sv.run_flagger_fused(fg, oracle, vis, masks["FULL"], "FULL", 13, True, 0,
                         sv.LONG if channels > 4096 else sv.STRIP)  # fmt: skip
    fg.check()


@pytest.mark.parametrize("far", turns("vis", "flags"), ids=ids)
def test_flagger_ring(far, gpu, arena, oracle):
    """The ring kernel takes no input flags and writes no deviations: vis and flags. With 4096
    rows of vis spread over more than 2**32 bytes its lane offsets do not fit 32 bits: the guard
    refuses it and the strip kernel does all the work."""
    vis, masks = sv.fused_inputs(4096, 12, 13)
    fg = FarGpu(gpu, arena, far)
    sv.run_flagger_fused(fg, oracle, vis, None, "NONE", 13, False, 1,
                         sv.STRIP if "vis" in far else sv.RING | sv.STRIP)  # fmt: skip
    fg.check()


# ------------------------------------------------- the launchers of the per-operation modules
def far_views(gpu, arena, far):
    return farviews.FarViews(arena, far, subviews.CompactViews(gpu.context, gpu.queue))


def with_groups(roles, *groups):
    """Each role far on its own, then the groups: all of the roles where one arena holds them,
    else the inputs, the outputs or the accumulators together."""
    return [(role,) for role in roles] + [tuple(group) for group in groups]


@pytest.mark.parametrize("far", turns("flags", "row_counts", "col_counts"), ids=ids)
@pytest.mark.parametrize("stride", [1007, 1008])
def test_flag_count(stride, far, gpu, arena):
    from tests import test_gpu_flag_count as module

    flags = module.sparse_flags(np.random.RandomState(stride), (37, 1003))
    masks = (0xFF, 0x10)
    views = far_views(gpu, arena, far)
    row_counts, col_counts = module.call_abi(gpu.context, gpu.queue, flags, stride, 0, masks, views)
    want_rows, want_cols = module.expected(flags, masks)
    np.testing.assert_array_equal(want_rows, row_counts)
    np.testing.assert_array_equal(want_cols, col_counts)
    views.check()


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("stride", [1007, 1008])
def test_sir(stride, axis, gpu, arena):
    from tests import test_gpu_sir as module

    rs = np.random.RandomState(stride)
    data = rs.randint(0, 256, (37, 1003)).astype(U8)
    data &= np.where(rs.random_sample(data.shape) < 0.85, 0xFE, 0xFF).astype(U8)
    views = far_views(gpu, arena, {"flags"})
    got = module.call_abi(gpu.context, gpu.queue, data, stride, 0, axis, 819, 0x01, 0x03, views)
    want = module.expected(data if axis == 0 else data.T, 819, 0x01, 0x03)
    np.testing.assert_array_equal(want if axis == 0 else want.T, got)
    assert (got != data).any()
    views.check()


AVERAGE_IN = ("vis", "flags", "weights", "mask")
AVERAGE_ACC = ("acc_vis", "acc_weights", "acc_flags")
AVERAGE_OUT = ("out_vis", "out_weights", "out_flags")


@pytest.mark.parametrize("far", with_groups(AVERAGE_IN + AVERAGE_ACC + AVERAGE_OUT, AVERAGE_IN,
                                            AVERAGE_ACC, AVERAGE_OUT), ids=ids)  # fmt: skip
def test_average(far, gpu, arena):
    """ksp_average_accumulate and ksp_average_finalise: 6 channels, averaged by 3; per-sample
    input flags, so that `mask` has rows."""
    from tests import test_gpu_average as module

    views = far_views(gpu, arena, far)
    module.check_raw_abi("FULL", 1, 37, gpu.context, gpu.queue, views)
    views.check()


@pytest.mark.parametrize("far", with_groups(AVERAGE_IN + AVERAGE_ACC, AVERAGE_IN, AVERAGE_ACC), ids=ids)
@pytest.mark.parametrize("aligned", [False, True])
def test_accumulate_block(aligned, far, gpu, arena):
    """Three dumps in a block; a single one where all four inputs are far (each dump has its
    own arrays, and one arena holds four of them)."""
    from tests import test_gpu_accumulate_block as module

    views = far_views(gpu, arena, far)
    strides, offset = (module.ALIGNED_STRIDES, 16) if aligned else (module.ODD_STRIDES, 1)
    module.check_raw_abi(gpu.context, gpu.queue, "FULL", 1 if len(far) == 4 else 3, 37, offset,
                         strides, make_views=views)  # fmt: skip
    views.check()


PREPARE = ("vis_in", "vis", "input_flags", "weights")


@pytest.mark.parametrize("far", with_groups(PREPARE, PREPARE), ids=ids)
@pytest.mark.parametrize("aligned", [False, True])
def test_prepare(aligned, far, gpu, arena):
    from tests import test_gpu_prepare as module

    views = far_views(gpu, arena, far)
    strides, offset = (module.ALIGNED_STRIDES, 16) if aligned else (module.ODD_STRIDES, 1)
    module.check_raw_abi(offset, strides, (True, True), 37, True, gpu.context, gpu.queue, views)
    views.check()


PREPARE_FLAGS = ("vis_in", "channel_flags", "vis", "input_flags", "weights")


@pytest.mark.parametrize("far", with_groups(PREPARE_FLAGS, PREPARE_FLAGS), ids=ids)
@pytest.mark.parametrize("aligned", [False, True])
def test_prepare_flags(aligned, far, gpu, arena):
    """Three classes of channel flags: `channel_flags` has three rows, as far apart as an int
    stride takes rows of bytes."""
    from tests import test_gpu_prepare_flags as module

    views = far_views(gpu, arena, far)
    strides, offset = (module.ALIGNED_STRIDES, 16) if aligned else (module.ODD_STRIDES, 1)
    module.check_raw_abi(offset, offset, strides, 3, True, True, gpu.context, gpu.queue, views)
    views.check()


@pytest.mark.parametrize("far", turns("weights", "weights8"), ids=ids)
@pytest.mark.parametrize("aligned", [False, True])
def test_compress_weights(aligned, far, gpu, arena):
    from tests import test_gpu_compress_weights as module

    views = far_views(gpu, arena, far)
    strides, offset = (module.aligned_strides, 16) if aligned else (module.odd_strides, 1)
    module.check_raw_abi(offset, strides, 6, 37, gpu.context, gpu.queue, views)
    views.check()


GAINS_IN = ("vis", "weights", "flags", "gains")
GAINS_OUT = ("out_vis", "out_weights", "out_flags")


@pytest.mark.parametrize("far", with_groups(GAINS_IN + GAINS_OUT, GAINS_IN, GAINS_OUT), ids=ids)
@pytest.mark.parametrize("aligned", [False, True])
def test_apply_gains(aligned, far, gpu, arena):
    """Out of place and in place (where the far inputs are the outputs)."""
    from tests import test_gpu_apply_gains as module

    views = far_views(gpu, arena, far)
    strides, offset = (module.aligned_strides, 16) if aligned else (module.odd_strides, 1)
    module.check_raw_abi(offset, strides, 6, 37, 5, gpu.context, gpu.queue, views, (True, True))
    views.check()


SOLVE_DATA = ("vis", "weights", "flags")
SOLVE_GAINS = ("pairs", "initial", "gains")


@pytest.mark.parametrize("far", with_groups(SOLVE_DATA + SOLVE_GAINS, SOLVE_DATA, SOLVE_GAINS), ids=ids)
def test_solve_gains(far, gpu, arena):
    """Apart from `initial` and in place (where the far `gains` are `initial` too)."""
    from tests import test_gpu_solve_gains as module

    views = far_views(gpu, arena, far)
    module.check_raw_abi(1, 6, 5, 0, gpu.context, gpu.queue, views, (True, True, True))
    views.check()


PREDICT_MODEL = ("delays", "flux", "model")
PREDICT_IN = ("vis", "weights", "flags")
PREDICT_OUT = ("out_vis", "out_weights", "out_flags")


@pytest.mark.parametrize("far", with_groups(PREDICT_MODEL + PREDICT_IN + PREDICT_OUT, PREDICT_MODEL,
                                            PREDICT_IN, PREDICT_OUT), ids=ids)  # fmt: skip
@pytest.mark.parametrize("aligned", [False, True])
def test_predict(aligned, far, gpu, arena):
    from tests import test_gpu_predict as module

    views = far_views(gpu, arena, far)
    strides, offset = (module.aligned_strides, 16) if aligned else (module.odd_strides, 1)
    module.check_raw_abi(offset, strides, 6, 37, 5, gpu.context, gpu.queue, views,
                         (True, True, True, True, False))  # fmt: skip
    views.check()


@pytest.mark.parametrize("far", turns("gains", "model"), ids=ids)
def test_fit_delays(far, gpu, arena):
    from tests import test_gpu_fit_delays as module

    views = far_views(gpu, arena, far)
    module.check_raw_abi(1, 6, 5, 16, gpu.context, gpu.queue, views, (True, True, True))
    views.check()


RANGE_IN = ("data", "flags")
RANGE_OUT = ("percentiles", "counts", "range_flags")


@pytest.mark.parametrize("far", with_groups(RANGE_IN + RANGE_OUT, RANGE_IN, RANGE_OUT), ids=ids)
@pytest.mark.parametrize("aligned", [False, True])
@pytest.mark.parametrize("dtype", [F32, C64])
def test_range_percentiles(dtype, aligned, far, gpu, arena):
    from tests import test_gpu_range_percentiles as module

    views = far_views(gpu, arena, far)
    strides, offset = (module.aligned_strides, 16) if aligned else (module.odd_strides, 1)
    module.check_raw_abi(offset, strides, True, dtype, gpu.context, gpu.queue, views)
    views.check()


BAND_IN = ("data", "flags", "channel_weights")
BAND_SUMS = ("mean", "mean_amplitude", "weight_sums")
BAND_COUNTS = ("counts", "series_flags")


@pytest.mark.parametrize("far", with_groups(BAND_IN + BAND_SUMS + BAND_COUNTS, BAND_IN, BAND_SUMS,
                                            BAND_COUNTS), ids=ids)  # fmt: skip
@pytest.mark.parametrize("aligned", [False, True])
def test_band_average(aligned, far, gpu, arena):
    from tests import test_gpu_band_average as module

    views = far_views(gpu, arena, far)
    strides, offset = (module.aligned_strides, 16) if aligned else (module.odd_strides, 1)
    module.check_raw_abi(offset, strides, True, gpu.context, gpu.queue, views)
    views.check()


# ------------------------------------------------ the 2-D flagger and the masked filter
# Their arrays are 3-D with two ``long long`` strides that data, flags and output share. Each
# stride is far in turn while the other one keeps its rows together, which makes the array a
# 2-D view: [outer][inner * cols] with the outer stride far, or [outer * inner][cols] with the
# inner stride far and the outer one a multiple of it. As with the thresholds, each type takes a
# turn at choosing the stride, as far as 32 GiB allow; every test asserts how far each of its
# arrays reached:
#
# * data choosing: its rows cross 2**32 bytes; the rows of the uint8 arrays then reach a quarter
#   (float32 data) or an eighth (complex64) of that, 1 GiB or 0.5 GiB;
# * flags choosing, masked filter: the flags cross 2**32 bytes, the float32 data 2**34 with
#   element offsets beyond 2**32 (24 GiB with its margin), in place, since a separate output of
#   that size does not fit;
# * flags choosing, 2-D flagger: on float32 amplitudes both flag arrays cross 2**31 bytes and
#   the data 2**33 with element offsets beyond 2**31 (16 + 4 + 4 GiB). Flags beyond 2**32 would
#   take 36 GiB, and with complex64 data flags beyond 2**31 would take 40 GiB.
G2, G4 = 2**31, 2**32


def three_d(views, role, array, far_axis, like, poison):
    """(view, outer stride, inner stride) of a 3-D `array` as a 2-D view with `like` as its
    stride, far along `far_axis` (0: outer, 1: inner)."""
    outer, inner, cols = array.shape
    flat = array.reshape((outer, inner * cols) if far_axis == 0 else (outer * inner, cols))
    view = views(role, array.dtype, flat, like, 0, poison)[0]
    assert isinstance(view, farviews.FarDeviceView)
    return view, (view.stride if far_axis == 0 else inner * view.stride), (
        cols if far_axis == 0 else view.stride)  # fmt: skip


def long_views(gpu, arena, far, span=farviews.SPAN):
    return farviews.FarViews(arena, far, subviews.CompactViews(gpu.context, gpu.queue), span,
                             farviews.LONG_STRIDE)  # fmt: skip


# (golden case, far roles, span asked for, least reach of data, least reach of either flags)
TWODFLAG_TURNS = [
    pytest.param("avg3", ("data",), farviews.SPAN, G4, G2 // 4, id="data"),
    pytest.param("amplitudes", ("in_flags", "out_flags"), G2 + 2**24, 2 * G4, G2, id="flags"),
]


@pytest.mark.parametrize("far_axis", [0, 1], ids=["stride_t", "stride_f"])
@pytest.mark.parametrize("name, far, span, data_reach, flags_reach", TWODFLAG_TURNS)
def test_twodflag(name, far, span, data_reach, flags_reach, far_axis, gpu, arena):
    """Golden cases, the reference's flags: avg3 (complex64, 32 x 100 x 2, channels averaged by
    3) with the data choosing the stride, amplitudes (float32, 32 x 96 x 2) with the flags."""
    from katsdpsigproc_amd.rfi import twodflag
    from tests import inputs_twodflag
    from tests import test_gpu_twodflag as module

    data, flags = inputs_twodflag.make_case(name)
    with np.load(inputs_twodflag.GOLDEN) as golden:
        want = module._expected(golden, name)
    n_time, n_freq, n_bl = data.shape
    template = twodflag.SumThresholdFlaggerDeviceTemplate(
        gpu.context, amplitudes=data.dtype == F32, **inputs_twodflag.CASES[name][3])
    op = template.instantiate(gpu.queue, n_time, n_freq, n_bl)
    views = long_views(gpu, arena, far, span)
    cols = n_freq * n_bl if far_axis == 0 else n_bl
    rows = n_time if far_axis == 0 else n_time * n_freq
    stride = views.shared_stride(cols + 6, [("data", rows, cols, data.dtype), ("in_flags", rows, cols, U8),
                                            ("out_flags", rows, cols, U8)])  # fmt: skip
    d_data, stride_t, stride_f = three_d(views, "data", data, far_axis, stride, True)
    d_in = three_d(views, "in_flags", flags.astype(U8), far_axis, stride, True)[0]
    d_out = three_d(views, "out_flags", subviews.sentinel_array(data.shape, U8), far_axis, stride, False)[0]
    assert d_in.stride == d_out.stride == d_data.stride
    assert d_data.reach > data_reach and d_in.reach > flags_reach and d_out.reach > flags_reach
    gpu.call("ksp_twodflag", d_data.ptr, d_in.ptr, d_out.ptr, n_bl, stride_t, stride_f, 0, op.batch,
             ctypes.byref(op.params), ctypes.c_void_p(op.workspace.buffer.ptr), op.workspace_bytes)  # fmt: skip
    got = d_out.read("out_flags").reshape(data.shape)
    assert want.any()
    np.testing.assert_array_equal(got.astype(np.bool_), want)
    assert set(np.unique(got)) <= {0, 1}
    d_data.read("data")
    d_in.read("in_flags")
    views.check()


# (far roles, in place, least reach of data and out, least reach of flags)
FILTER_TURNS = [
    pytest.param(("data",), False, G4, G2 // 2, id="data"),
    pytest.param(("data",), True, G4, G2 // 2, id="data-in-place"),
    pytest.param(("flags",), True, 4 * G4, G4, id="flags-in-place"),
]


@pytest.mark.parametrize("far_axis", [0, 1], ids=["image_stride", "row_stride"])
@pytest.mark.parametrize("far, in_place, data_reach, flags_reach", FILTER_TURNS)
def test_masked_filter(far, in_place, data_reach, flags_reach, far_axis, gpu, arena):
    """Three images of 40 x 48 float32, box radii 2 and 7, against the NumPy restatement."""
    from katsdpsigproc_amd.rfi import twodflag
    from tests import inputs_masked_filter, masked_filter_oracle
    from tests import test_gpu_masked_filter as module

    images, rows, cols = 3, 40, 48
    sigma = (module.SIGMA_R2, module.SIGMA_R7)
    pairs = [inputs_masked_filter.make_inputs((rows, cols), F32, "lognormal", "sparse", 30 + k)
             for k in range(images)]  # fmt: skip
    data = np.stack([p[0] for p in pairs])
    flags = np.stack([p[1] for p in pairs]).astype(U8)
    want = masked_filter_oracle.masked_filter(data, flags, sigma, 4)
    op = twodflag.MaskedGaussianFilterTemplate(gpu.context, F32, 4).instantiate(gpu.queue, data.shape, sigma)
    views = long_views(gpu, arena, far)
    width = rows * cols if far_axis == 0 else cols
    height = images if far_axis == 0 else images * rows
    sharing = [("data", height, width, F32), ("flags", height, width, U8)]
    stride = views.shared_stride(width + 5, sharing + ([] if in_place else [("out", height, width, F32)]))
    # in place the data is an output: sentinels around it instead of poison
    d_data, image_stride, row_stride = three_d(views, "data", data, far_axis, stride, not in_place)
    d_flags = three_d(views, "flags", flags, far_axis, stride, True)[0]
    d_out = d_data if in_place else three_d(
        views, "out", subviews.sentinel_array(data.shape, F32), far_axis, stride, False)[0]  # fmt: skip
    assert d_data.reach > data_reach and d_out.reach > data_reach and d_flags.reach > flags_reach
    gpu.call("ksp_masked_filter", d_data.ptr, d_flags.ptr, d_out.ptr, rows, cols, images,
             image_stride, row_stride, 0, op.batch, op.radii[0], op.radii[1], 4, op.divisors[0],
             op.divisors[1], 4, ctypes.c_void_p(op.workspace.buffer.ptr), op.workspace_bytes)  # fmt: skip
    module._same(d_out.read("out").reshape(data.shape), want)
    assert flags.any() and not flags.all() and not np.isnan(want).all()
    if not in_place:
        d_data.read("data")
    d_flags.read("flags")
    views.check()


# --------------------------------------------------- the ring kernel at the edge of its guard
def ring_guard_vis():
    """Noise, 4096 channels x 21 baselines (two strips of 8 and a tail of 5), with the special
    values of test_gpu_ring_pipeline.py in every baseline of both strips."""
    from tests import test_gpu_ring_pipeline as ring

    vis = inputs.generate_data(4096, 21, seed=5)
    for b in range(16):
        value = ring.SPECIALS[b % len(ring.SPECIALS)]
        offset = ring.OFFSETS[(b // len(ring.SPECIALS) + b) % len(ring.OFFSETS)]
        lane = (0, 63)[b % 2] if b % 5 == 0 else (11 * b + 1) % 64
        vis[ring.RUN * lane + offset, b] = value
    return vis


@pytest.mark.parametrize("vis_stride, path", [(65534, sv.RING | sv.STRIP), (65536, sv.STRIP)])
def test_ring_guard(vis_stride, path, gpu, arena, oracle):
    """The largest even vis_stride the ring kernel's guard admits (65534 * 8 * 4096 <
    0x7fffff00: the lane offsets reach 4032 rows * 524272 B, just under 2**31) and the first it
    refuses. flags are far as well. Launched twice, as the ring tests do: the second launch finds
    the scheduling counters as the first left them."""
    from katsdpsigproc_amd import accel

    vis = ring_guard_vis()
    channels, baselines = vis.shape
    with np.errstate(all="ignore"):
        want_flags, want_noise = oracle.flagger_full(vis, width=13, n_sigma=11.0, n_windows=4)
    assert want_flags.any()
    fg = FarGpu(gpu, arena, {"flags"})
    d_vis = fg.input(vis, vis_stride, role="vis")
    assert isinstance(d_vis, farviews.FarDeviceView) and d_vis.address % 16 == 0
    d_flags = fg.output(vis.shape, U8, baselines + 5, role="flags")
    d_noise = fg.output(baselines, F32, offset=1)
    workspace = accel.DeviceArray(gpu.context, (16,), np.uint32)
    workspace.zero(gpu.queue)
    for launch in (1, 2):
        with _lib.fused_ring_mode(1):
            fg.call("ksp_flagger_fused", d_vis.ptr, None, d_flags.ptr, None, d_noise.ptr, channels,
                    baselines, d_vis.stride, 0, d_flags.stride, 0, 13, 0, 0, 1, 11.0,
                    sv.FUSED_SCALES, 4, 1, ctypes.c_void_p(workspace.buffer.ptr))  # fmt: skip
            assert _lib.call("ksp_flagger_fused_last_path") == path
        what = f"vis_stride {vis_stride}, launch {launch}"
        sv.assert_equal(want_flags, d_flags.read("flags, " + what), "flags, " + what)
        sv.assert_equal(want_noise.astype(F32)[np.newaxis], d_noise.read("noise"), "noise, " + what)
    d_vis.read("vis")
    assert not workspace.get(gpu.queue).any(), "the workspace was not left zeroed"
    fg.check()


# ------------------------------------------------------------------ region copies of accel
def test_region_copies(gpu, arena):
    """set_region, copy_region and get_region on complex64 (3, 8) arrays padded to rows of
    2**29 + 16 elements: origins and pitches beyond 2**32 bytes in ksp_memcpy_rect_async. The
    two arrays are slices of the arena, full of sentinels; the audit counts what was written."""
    from katsdpsigproc_amd import accel

    shape, padded = (3, 8), (3, 2**29 + 16)
    n_bytes = farviews.up16(padded[0] * padded[1] * 8 // 256 + 1) * 256
    arena.reset()
    arrays = []
    for _ in range(2):
        raw = farviews.BorrowedBuffer(arena.device, arena.take(n_bytes), n_bytes)
        arrays.append(accel.DeviceArray(gpu.context, shape, C64, padded, raw=raw))
    first, second = arrays
    assert first.strides[0] > 2**32
    rs = np.random.RandomState(8)
    data = (rs.standard_normal(shape) + 1j * rs.standard_normal(shape)).astype(C64)
    first.set_region(gpu.queue, data, np.s_[:, :], np.s_[:, :])
    first.copy_region(gpu.queue, second, np.s_[:, 1:7], np.s_[:, 2:8])
    for array, region, want in [(first, np.s_[:, :], data), (second, np.s_[:, 2:8], data[:, 1:7])]:
        got = accel.HostArray(want.shape, C64, context=gpu.context)
        array.get_region(gpu.queue, got, region, np.s_[:, :])
        np.testing.assert_array_equal(want.view(np.uint8), np.asarray(got).view(np.uint8))
        written = int(np.count_nonzero(np.ascontiguousarray(want).view(np.uint8) != subviews.SENTINEL))
        assert arena.count(array.buffer.ptr, n_bytes) == written, "bytes outside the region were written"
