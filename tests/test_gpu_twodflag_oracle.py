"""2-D flagger on the GPU against the NumPy oracle, bit for bit: the final flags and every
stage the workspace holds after the last batch (``ksp_twodflag_layout``), on every golden
case, at production shapes aimed at the kernels' branches, and on blocks of edge baselines."""

import ctypes

import numpy as np
import pytest

from katsdpsigproc_amd import _lib, accel
from katsdpsigproc_amd.rfi import twodflag
from oracle import twodflag_oracle as oracle
from tests import inputs_twodflag as inputs

pytestmark = pytest.mark.gpu

#: 32 frequency windows, up to 384 channels (halos over three chunks of 128)
WINDOWS_FREQ_32 = list(range(1, 25)) + [32, 48, 64, 96, 128, 192, 256, 384]

#: name -> (shape, kind, amplitudes, keywords, batch, padding (channels, baselines))
PRODUCTION = {
    # chunks of about 410 channels: the radix select runs over ~105 k values per workgroup
    "dense": ((256, 4096, 4), "rfi", False, {}, None, None),
    # the longest lines, the widest time box (radius 2047), 32 time windows
    "long_time": ((4096, 48, 2), "amplitudes", True,
                  {"spike_width_time": 2364.0, "windows_time": inputs.WINDOWS_TIME_32},
                  None, None),
    # the widest band, 512 chunks, radius 2047 along frequency, 32 frequency windows
    "wide_band": ((8, 65536, 2), "rfi", False,
                  {"freq_chunks": 512, "spike_width_freq": 2364.0,
                   "windows_freq": WINDOWS_FREQ_32}, None, None),
    # ragged averaging groups, 37 chunks, even extends, whole rows and whole channels
    "averaged": ((64, 30001, 3), "rfi", False,
                 {"average_freq": 7, "freq_chunks": 37, "time_extend": 4, "freq_extend": 6,
                  "flag_all_time_frac": 0.3, "flag_all_freq_frac": 0.3}, None, None),
    # batches of 8 with a ragged last one, padded axes, 3 background iterations
    "batched": ((128, 2048, 37), "rfi", False, {"background_iterations": 3}, 8, (5, 3)),
}  # fmt: skip


@pytest.fixture(scope="module")
def context():
    return accel.create_some_context(interactive=False)


@pytest.fixture(scope="module")
def queue(context):
    return context.create_command_queue()


def run_device(context, queue, data, flags, kw, batch=None, padding=None):
    """Flags of the device operation and the stages of its last batch:
    (flags (time, channel, baseline) uint8, first baseline of the last batch, stages)."""
    template = twodflag.SumThresholdFlaggerDeviceTemplate(
        context, amplitudes=data.dtype == np.float32, **kw)
    op = template.instantiate(queue, *data.shape, batch=batch)
    if padding is not None:
        dims = op.slots["data"].dimensions
        for axis, extra in zip((1, 2), padding):
            n = data.shape[axis]
            dims[axis].link(accel.Dimension(n, min_padded_size=n + extra))
    op.ensure_all_bound()
    op.buffer("data").set(queue, data)
    op.buffer("input_flags").set(queue, flags)
    op()
    out = op.buffer("flags").get(queue)
    workspace = op.workspace.get(queue)
    n_bl = data.shape[2]
    last = (n_bl - 1) // op.batch * op.batch
    nb = n_bl - last
    offsets = _lib.TwodflagOffsets()
    _lib.call("ksp_twodflag_layout", ctypes.byref(op.params), nb, ctypes.byref(offsets))
    T, F = data.shape[:2]
    dims = {"B": nb, "T": T, "A": op.params.chunk_ends[op.params.n_chunks], "F": F}
    stages = {}
    for name, (dtype, axes) in oracle.STAGES.items():
        shape = tuple(dims[c] for c in axes)
        start = getattr(offsets, name)
        size = int(np.prod(shape)) * np.dtype(dtype).itemsize
        stages[name] = workspace[start:start + size].view(dtype).reshape(shape)
    return out, last, stages


def assert_matches_oracle(data, flags, kw, out, last, stages, label):
    expected, ref = oracle.flag(data, flags, **kw)
    assert out.dtype == np.uint8 and set(np.unique(out)) <= {0, 1}
    diff = out.astype(np.bool_) != expected
    assert not diff.any(), f"{label}: {int(diff.sum())} flags differ"
    for name, (dtype, _) in oracle.STAGES.items():
        theirs, mine = stages[name], ref[name][last:]
        if dtype == np.float32:
            same = np.array_equal(theirs.view(np.uint32), mine.view(np.uint32))
        else:
            same = np.array_equal(theirs, mine)
        assert same, f"{label}: stage {name} differs at {int((theirs != mine).sum())} places"


@pytest.mark.parametrize("name", sorted(inputs.CASES))
def test_golden_case_stages(context, queue, name):
    shape, _, _, kw = inputs.CASES[name]
    data, flags = inputs.make_case(name)
    out, last, stages = run_device(context, queue, data, flags.astype(np.uint8), kw)
    assert last == 0
    assert_matches_oracle(data, flags, kw, out, last, stages, name)


@pytest.mark.parametrize("name", list(PRODUCTION))
def test_production_shape(context, queue, name):
    shape, kind, amplitudes, kw, batch, padding = PRODUCTION[name]
    data, flags = inputs.make_data(shape, kind, 41, amplitudes)
    out, last, stages = run_device(context, queue, data, flags.astype(np.uint8), kw, batch,
                                   padding)  # fmt: skip
    if batch is not None:
        assert last == shape[2] // batch * batch  # the ragged last batch's stages
    assert_matches_oracle(data, flags, kw, out, last, stages, name)


@pytest.mark.parametrize("amplitudes", [False, True], ids=["complex64", "float32"])
def test_edge_baselines(context, queue, amplitudes):
    """Quantised, constant, all-zero, subnormal, very large, negative and half-NaN
    baselines side by side; input flags given as the bytes 1, 2, 128 and 255."""
    n_bl = len(inputs.EDGE_KINDS[amplitudes]) * 2
    data, flags = inputs.edge_block((96, 1024, n_bl), amplitudes, 500)
    rs = np.random.RandomState(7)
    flags = flags | (rs.random_sample(flags.shape) < 0.02)
    raw = np.where(flags, rs.choice(np.array([1, 2, 128, 255], np.uint8), flags.shape), 0)
    raw = raw.astype(np.uint8)
    assert set(np.unique(raw)) == {0, 1, 2, 128, 255}
    kw = {"freq_chunks": 7, "time_extend": 2, "freq_extend": 2}
    out, last, stages = run_device(context, queue, data, raw, kw)
    assert_matches_oracle(data, flags, kw, out, last, stages, "edges")
