"""masked_gaussian_filter on the GPU: the reference's results bit for bit (golden cases),
the NumPy restatement everywhere else, batching and padding, the host function, and the
reference test's acceptance properties."""

import numpy as np
import pytest

from katsdpsigproc_amd import accel
from katsdpsigproc_amd.rfi import twodflag
from tests import inputs_masked_filter as inputs
from tests import masked_filter_oracle as oracle

pytestmark = pytest.mark.gpu

#: sigma whose 4-pass box radius is 2, 7 and 34
SIGMA_R2, SIGMA_R7, SIGMA_R34 = 2.3, 8.5, 40.0
SENTINEL = -7.5


@pytest.fixture(scope="module")
def context():
    return accel.create_some_context(interactive=False)


@pytest.fixture(scope="module")
def queue(context):
    return context.create_command_queue()


@pytest.fixture(scope="module")
def golden():
    with np.load(inputs.GOLDEN) as g:
        return {k: g[k] for k in g.files}


def _device_filter(context, queue, data, flags, sigma, passes=4, batch=None, pad=None,
                   in_place=False):  # fmt: skip
    """The device operation's result; with `pad` the slots get that padded shape and the
    padding of `out` is checked to be left alone."""
    template = twodflag.MaskedGaussianFilterTemplate(context, data.dtype, passes)
    op = template.instantiate(queue, data.shape, sigma, batch=batch)
    if pad is not None:
        for dim, size, padded in zip(op.slots["data"].dimensions, data.shape, pad):
            dim.link(accel.Dimension(size, min_padded_size=padded))
    op.ensure_all_bound()
    if in_place:
        op.bind(out=op.buffer("data"))
    op.buffer("data").set(queue, data)
    op.buffer("flags").set(queue, flags.astype(np.uint8) if flags.dtype == np.bool_ else flags)
    if not in_place:
        staged = op.buffer("out").empty_like()
        accel.HostArray.padded_view(staged)[...] = SENTINEL
        op.buffer("out").set(queue, staged)
    op()
    out = op.buffer("out").get(queue)
    if pad is not None:
        assert op.buffer("out").padded_shape == tuple(pad)
    if not in_place:
        whole = accel.HostArray.padded_view(out)
        outside = np.ones(whole.shape, np.bool_)
        outside[tuple(slice(0, s) for s in data.shape)] = False
        assert np.all(whole[outside] == SENTINEL), "padding of out was written"
    return np.array(out)


def _same(out, expected):
    assert out.dtype == expected.dtype and out.shape == expected.shape
    nan = np.isnan(expected)
    assert np.array_equal(np.isnan(out), nan), "NaN positions differ"
    differ = int((out[~nan] != expected[~nan]).sum())
    assert differ == 0, f"{differ} of {expected.size} values differ"


def _check(context, queue, data, flags, sigma, passes=4, **kw):
    out = _device_filter(context, queue, data, flags, sigma, passes, **kw)
    _same(out, oracle.masked_filter(data, flags, sigma, passes))
    return out


@pytest.mark.parametrize("name", sorted(inputs.CASES))
def test_golden(context, queue, golden, name):
    """The reference's own results: both types, passes 1..8, radii (0, r), (r, 0), (0, 0),
    boxes wider than the line, the divisor 69 ** 4 on either axis."""
    _shape, _dtype, sigma, passes = inputs.CASES[name][:4]
    data, flags = inputs.make_case(name)
    out = _device_filter(context, queue, data, flags, sigma, passes)
    _same(out, golden[name])
    if name == "block":
        nan = np.isnan(out).mean()
        assert nan > 0.01 and 1 - nan > 0.5
    if name == "copy":
        assert np.array_equal(np.isnan(out), flags)
        assert np.array_equal(out[~flags], data[~flags])
    if name.startswith("d69"):
        assert inputs.radius(max(sigma), passes) == 34


@pytest.mark.parametrize("shape", [(1, 50), (50, 1), (1, 1), (1, 300), (300, 1)])
@pytest.mark.parametrize("sigma", [SIGMA_R2, SIGMA_R7])
def test_single_lines(context, queue, shape, sigma):
    data, flags = inputs.make_inputs(shape, np.float32, "lognormal", "sparse", 21)
    _check(context, queue, data, flags, (sigma, sigma))


# 64 lanes a wavefront, 256 lines a workgroup (130 rows x 2 arrays: two of them), LDS tiles
# of 32 float32 / 16 float64 columns
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", [(64, 64), (65, 63), (130, 67), (67, 130), (257, 33), (40, 300)])
@pytest.mark.parametrize("sigma", [SIGMA_R2, SIGMA_R7])
def test_tile_and_wavefront_edges(context, queue, dtype, shape, sigma):
    data, flags = inputs.make_inputs(shape, dtype, "lognormal", "sparse", 22)
    _check(context, queue, data, flags, (sigma, sigma))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("sigma", [SIGMA_R2, SIGMA_R7, SIGMA_R34])
def test_summation_order(context, queue, dtype, sigma):
    """Amplitudes over many binades: a prefix-sum or windowed formulation of the same
    filter rounds differently on these (on uniform data it mostly would not)."""
    data, flags = inputs.make_inputs((64, 300), dtype, "lognormal", "none", 23)
    assert inputs.radius(sigma, 4) in (2, 7, 34)
    _check(context, queue, data, flags, (0.0, sigma))
    _check(context, queue, np.ascontiguousarray(data.T), flags.T, (sigma, 0.0))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("passes", [1, 2, 3, 5, 8])
def test_passes(context, queue, dtype, passes):
    data, flags = inputs.make_inputs((45, 52), dtype, "lognormal", "half", 24)
    _check(context, queue, data, flags, (3.0, 4.0), passes)


def test_one_pass_radius_equal_to_length(context, queue):
    data, flags = inputs.make_inputs((6, 6), np.float64, "lognormal", "sparse", 25)
    assert inputs.radius(3.5, 1) == 6
    _check(context, queue, data, flags, (3.5, 3.5), 1)


def test_flag_values(context, queue):
    shape = (33, 47)
    data = inputs.make_data(shape, np.float32, "lognormal", 26)
    none = np.zeros(shape, np.bool_)
    out = _check(context, queue, data, none, (SIGMA_R2, SIGMA_R7))
    assert np.all(np.isfinite(out))
    out = _check(context, queue, data, ~none, (SIGMA_R2, SIGMA_R7))
    assert np.all(np.isnan(out))
    # any non-zero byte flags
    rs = np.random.RandomState(27)
    flags = rs.choice(np.array([0, 0, 1, 2, 128, 255], np.uint8), size=shape)
    expected = oracle.masked_filter(data, flags != 0, (SIGMA_R2, SIGMA_R7))
    _same(_device_filter(context, queue, data, flags, (SIGMA_R2, SIGMA_R7)), expected)


def test_batches_and_padding(context, queue):
    """5 images in batches of 2 (the last one ragged), slots padded on both axes: equal to
    5 single-image calls, the padding of out untouched."""
    shape = (5, 40, 70)
    data, flags = inputs.make_inputs(shape, np.float32, "lognormal", "half", 28)
    sigma = (5.0, SIGMA_R2)
    out = _check(context, queue, data, flags, sigma, batch=2, pad=(5, 48, 96))
    for k in range(5):
        single = _device_filter(context, queue, data[k], flags[k], sigma)
        _same(out[k], single)
    _same(_device_filter(context, queue, data, flags, sigma), out)  # one batch
    _same(_device_filter(context, queue, data, flags, sigma, batch=2, in_place=True), out)
    # rows longer than the alignment hint are padded by the slots themselves
    wide, wflags = inputs.make_inputs((2, 20, 200), np.float64, "lognormal", "half", 29)
    _check(context, queue, wide, wflags, (SIGMA_R2, 5.0), batch=1)


def test_host_function(context):
    data, flags = inputs.make_inputs((77, 53), np.float32, "lognormal", "half", 30)
    sigma = (5.0, SIGMA_R2)
    expected = oracle.masked_filter(data, flags, sigma)
    data0, flags0 = data.copy(), flags.copy()
    out = np.full_like(data, SENTINEL)
    assert twodflag.masked_gaussian_filter(data, flags, sigma, out, context=context) is None
    _same(out, expected)
    assert np.array_equal(data, data0) and np.array_equal(flags, flags0)
    # uint8 (and wider) flags, any non-zero value
    for dtype in (np.uint8, np.int32):
        out[...] = SENTINEL
        twodflag.masked_gaussian_filter(data, flags.astype(dtype) * 3, sigma, out, context=context)
        _same(out, expected)
    # out is data
    work = data.copy()
    twodflag.masked_gaussian_filter(work, flags, sigma, work, context=context)
    _same(work, expected)
    # non-contiguous data, flags and out
    big = np.zeros((77, 2 * 53), np.float32)
    big[:, ::2] = data
    big_flags = np.ones((2 * 77, 53), np.bool_)
    big_flags[1::2] = flags
    big_out = np.full((53, 77), SENTINEL, np.float32)
    twodflag.masked_gaussian_filter(big[:, ::2], big_flags[1::2], sigma, big_out.T, context=context)
    _same(np.ascontiguousarray(big_out.T), expected)
    # scalar sigma, float64, other passes
    data64 = data.astype(np.float64)
    out64 = np.empty_like(data64)
    twodflag.masked_gaussian_filter(data64, flags, 3.0, out64, 3, context=context)
    _same(out64, oracle.masked_filter(data64, flags, (3.0, 3.0), 3))
    twodflag.masked_gaussian_filter(data64, flags, [3.0], out64, passes=2, context=context)
    _same(out64, oracle.masked_filter(data64, flags, (3.0, 3.0), 2))


def test_host_function_keeps_its_context():
    data, flags = inputs.make_inputs((20, 30), np.float32, "uniform", "sparse", 31)
    out = np.empty_like(data)
    twodflag.masked_gaussian_filter(data, flags, (2.0, 2.0), out)
    _same(out, oracle.masked_filter(data, flags, (2.0, 2.0)))
    first = twodflag._filter_context
    assert first is not None
    queue = twodflag._filter_queue(None)[1]
    twodflag.masked_gaussian_filter(data, flags, (2.0, 2.0), out)
    assert twodflag._filter_context is first and twodflag._filter_queue(None)[1] is queue


def test_impulse_response(context, queue):
    """The reference's acceptance test of the box approximation: symmetric, unit sum,
    standard deviation within 1 of sigma."""
    data = np.zeros((1, 200), np.float32)
    data[0, 100] = 1.0
    out = _check(context, queue, data, np.zeros(data.shape, np.bool_), (0.0, 10.0))[0]
    assert np.array_equal(out[1:], out[:0:-1])  # out[100 + k] == out[100 - k]
    total = out.astype(np.float64).sum()
    assert abs(total - 1.0) < 1e-5
    x = np.arange(200) - 100.0
    assert abs((out * x).sum()) < 1e-5
    std = np.sqrt((out * x * x).sum() / total)
    assert abs(std - 10.0) < 1.0


def test_axes_are_interchangeable(context, queue):
    """Filtering along axis 0 equals filtering the transposed image along axis 1."""
    data, flags = inputs.make_inputs((70, 45), np.float32, "lognormal", "half", 32)
    for sigma in (SIGMA_R2, SIGMA_R7):
        a = _device_filter(context, queue, data, flags, (sigma, 0.0))
        b = _device_filter(context, queue, np.ascontiguousarray(data.T),
                           np.ascontiguousarray(flags.T), (0.0, sigma))  # fmt: skip
        _same(a, np.ascontiguousarray(b.T))
