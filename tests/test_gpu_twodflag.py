"""2-D SumThreshold flagger on the GPU: the reference's flags bit for bit (golden cases),
the reference test's acceptance properties, batching, large blocks."""

import numpy as np
import pytest

from katsdpsigproc_amd import accel
from katsdpsigproc_amd.rfi import twodflag
from tests import inputs_twodflag as inputs

pytestmark = pytest.mark.gpu


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


def _expected(golden, name):
    shape = inputs.CASES[name][0]
    bits = np.unpackbits(golden[name + "_flags"])[: int(np.prod(shape))]
    return bits.reshape(shape).astype(np.bool_)


def _device_flags(context, queue, data, flags, batch=None, **kw):
    amplitudes = data.dtype == np.float32
    template = twodflag.SumThresholdFlaggerDeviceTemplate(context, amplitudes=amplitudes, **kw)
    op = template.instantiate(queue, *data.shape, batch=batch)
    op.ensure_all_bound()
    op.buffer("data").set(queue, data)
    op.buffer("input_flags").set(queue, flags.astype(np.uint8))
    op()
    return op.buffer("flags").get(queue).astype(np.bool_)


@pytest.mark.parametrize("name", sorted(inputs.CASES))
def test_golden_device_operation(context, queue, golden, name):
    data, flags = inputs.make_case(name)
    params = inputs.CASES[name][3]
    out = _device_flags(context, queue, data, flags, **params)
    expected = _expected(golden, name)
    assert np.array_equal(out, expected), f"{int((out != expected).sum())} flags differ"


@pytest.mark.parametrize("name", sorted(inputs.CASES))
def test_golden_host_class(context, golden, name):
    data, flags = inputs.make_case(name)
    flagger = twodflag.SumThresholdFlagger(context=context, **inputs.CASES[name][3])
    out = flagger.get_flags(data, flags, chunk_size=1)
    assert out.dtype == np.bool_
    np.testing.assert_array_equal(out, _expected(golden, name))


def _bandpass(shape, rs):
    n_time, n_freq, n_bl = shape
    nx = 10
    x = np.linspace(0.0, n_freq, nx)
    y = np.ones((n_time, nx, n_bl)) * 2.34
    y[:, 0, :] = 0.1
    y[:, -1, :] = 0.1
    y[:] += rs.uniform(0.0, 0.1, y.shape)
    try:
        import scipy.interpolate

        f = scipy.interpolate.interp1d(x, y, axis=1, kind="cubic", assume_sorted=True)
        return f(np.arange(n_freq))
    except ImportError:
        # linear between the knots, then smoothed: a bandpass smooth on the filter's scale
        lin = np.stack([np.stack([np.interp(np.arange(n_freq), x, y[t, :, b])
                                  for b in range(n_bl)], axis=-1) for t in range(n_time)])  # fmt: skip
        k = np.ones(31) / 31
        pad = np.pad(lin, ((0, 0), (15, 15), (0, 0)), mode="edge")
        return np.apply_along_axis(lambda v: np.convolve(v, k, mode="valid"), 1, pad)


def _acceptance_data(average_freq, rs, shape=(234, 345, 1)):
    """The reference test's block (test/rfi/test_twodflag.py:531-569)."""
    data = _bandpass(shape, rs).astype(np.float32)
    data += (rs.standard_normal(shape) * 0.1).astype(np.float32)
    rfi = np.zeros(shape, np.float32)
    rfi[12, :] = 1
    rfi[20:25, :] = 1
    rfi[:, 17] = 1
    rfi[:, 200:220] = 1
    rfi[30, :300] = 1
    rfi[50:, 80] = 1
    rfi[60:65, 100:170] = 1
    rfi[150:200, 150:153] = 1
    expected = rfi.astype(np.bool_)
    expected[30, :] = True
    expected[:, 80] = True
    data += rfi * rs.standard_normal(shape) * 3.0
    data[:, 260] += 0.2 * average_freq
    expected[:, 260] = True
    data[225, 225] = np.nan
    expected[225, 225] = True
    in_flags = np.zeros(shape, np.bool_)
    in_flags[:, 185:190] = True
    data[:, 185:190] = np.nan
    return np.abs(data), in_flags, expected


@pytest.mark.parametrize("kw", [{}, {"freq_chunks": 1}, {"freq_chunks": 15}, {"average_freq": 2}])
def test_acceptance(context, kw):
    """Every expected flag set, fewer than 3 % extra outside the allowed band (the reference
    skips its background_iterations=3 case, and so does this)."""
    rs = np.random.RandomState(seed=1)
    data, in_flags, expected = _acceptance_data(kw.get("average_freq", 1), rs)
    orig_data, orig_flags = data.copy(), in_flags.copy()
    flagger = twodflag.SumThresholdFlagger(context=context, **kw)
    out = flagger.get_flags(data, in_flags)
    np.testing.assert_array_equal(data, orig_data)
    np.testing.assert_array_equal(in_flags, orig_flags)
    allowed = expected | in_flags
    allowed[:-1] |= allowed[1:]
    allowed[1:] |= allowed[:-1]
    allowed[:, :-1] |= allowed[:, 1:]
    allowed[:, 1:] |= allowed[:, :-1]
    allowed[:, :40] = True
    allowed[:, -40:] = True
    assert (expected & ~out).sum() == 0
    assert (out & ~allowed).sum() / data.size < 0.03


@pytest.mark.parametrize("kw", [{}, {"average_freq": 4}])
def test_all_flagged_gives_no_flags(context, kw):
    data = np.zeros((100, 80, 4), np.float32)
    out = twodflag.SumThresholdFlagger(context=context, **kw).get_flags(
        data, np.ones(data.shape, np.bool_))
    assert not out.any()


def test_chunk_size_and_inputs_unchanged(context):
    data, flags = inputs.make_case("odd")
    d0, f0 = data.copy(), flags.copy()
    flagger = twodflag.SumThresholdFlagger(context=context, **inputs.CASES["odd"][3])
    results = [flagger.get_flags(data, flags, chunk_size=c) for c in (None, 1, 2, 16)]
    for r in results[1:]:
        np.testing.assert_array_equal(r, results[0])
    np.testing.assert_array_equal(data, d0)
    np.testing.assert_array_equal(flags, f0)


def test_nan_propagates(context):
    data, flags = inputs.make_case("default")
    data = data.copy()
    data[3, 7, 1] = complex(np.nan, 0.0)
    data[5, 9, 0] = complex(0.0, np.nan)
    out = twodflag.SumThresholdFlagger(context=context).get_flags(data, flags)
    assert out[3, 7, 1] and out[5, 9, 0]


def test_padded_slots(context, queue, golden):
    """Channel and baseline axes padded by the caller: every slot shares the padding."""
    name = "avg3"
    data, flags = inputs.make_case(name)
    data, flags = np.tile(data, (1, 1, 20)), np.tile(flags, (1, 1, 20))
    template = twodflag.SumThresholdFlaggerDeviceTemplate(context, **inputs.CASES[name][3])
    op = template.instantiate(queue, *data.shape, batch=7)
    dims = op.slots["data"].dimensions
    dims[1].link(accel.Dimension(data.shape[1], min_padded_size=data.shape[1] + 3))
    dims[2].link(accel.Dimension(data.shape[2], min_padded_size=data.shape[2] + 5))
    op.ensure_all_bound()
    assert op.buffer("data").padded_shape[2] > data.shape[2]
    assert op.buffer("flags").padded_shape == op.buffer("data").padded_shape
    op.buffer("data").set(queue, data)
    op.buffer("input_flags").set(queue, flags.astype(np.uint8))
    op()
    out = op.buffer("flags").get(queue).astype(np.bool_)
    np.testing.assert_array_equal(out, np.tile(_expected(golden, name), (1, 1, 20)))


def test_large_block_matches_subset(context):
    rs = np.random.RandomState(seed=99)
    shape = (100, 4096, 2016)
    data = np.empty(shape, np.complex64)
    band = inputs.bandpass(1, shape[1], shape[2], rs)[0]
    for t in range(shape[0]):
        data[t] = band + (rs.standard_normal(shape[1:]) * 0.1).astype(np.float32)
    data[rs.randint(0, 100, 5000), rs.randint(0, 4096, 5000), rs.randint(0, 2016, 5000)] += 3.0
    flags = np.zeros(shape, np.bool_)
    flags[:, 1000:1010] = True
    flagger = twodflag.SumThresholdFlagger(context=context)
    out = flagger.get_flags(data, flags)
    sample = np.sort(rs.choice(shape[2], 8, replace=False))
    sub = flagger.get_flags(np.ascontiguousarray(data[..., sample]),
                            np.ascontiguousarray(flags[..., sample]))  # fmt: skip
    np.testing.assert_array_equal(out[..., sample], sub)
    assert out[..., sample].any()
    # and the sampled baselines are what the NumPy oracle computes for them
    from oracle import twodflag_oracle as oracle

    expected, _ = oracle.flag(np.ascontiguousarray(data[..., sample]),
                              np.ascontiguousarray(flags[..., sample]))  # fmt: skip
    np.testing.assert_array_equal(out[..., sample], expected)
