"""Filling solved gains across flagged channels on the GPU
(``rfi.ingest.InterpolateGainsTemplate``, ``ksp_interpolate_gains``): every comparison is of
bit patterns, of all outputs, against ``rfi.host.InterpolateGainsHost``, with nothing left out
but the payload of a NaN that the host has as a NaN too."""

import ctypes
import functools
import itertools

import numpy as np
import pytest

from tests import inputs_interpolate_gains as gen
from tests.inputs_interpolate_gains import assert_same
from tests.subviews import CompactViews, poison_array, sentinel_array

pytestmark = pytest.mark.gpu

# The sizes at which csrc/interpolate_gains.hip changes path. The workgroup has as many threads
# as the next power of two at or above the channels, at least 64 (one wavefront: 1, 2, 3 and up
# to 64 channels) and at most 1024, so the thread count steps behind 64, 128, 256 and 512
# channels, and with it the number of wavefronts whose ballots make the words of kept bits (one
# wavefront scans them up to 4096 channels, two to four above) and the levels of the amplitude's
# tree that cross wavefronts. From 1025 channels on a thread owns ceil(channels / 1024) channels,
# one more behind every multiple of 1024 up to 16 at 16384, and the tree's thread-local levels
# are those of the next power of two (2, 4, 8, 16 terms). Each group below is one step: one
# channel below it, at it and one above.
STEPS = [[1, 2, 3]] + [[n - 1, n, n + 1] for n in (64, 128, 256, 512)] + [
    [1024 * k - 1, 1024 * k, 1024 * k + 1] for k in range(1, 16)] + [[16383, 16384]]  # fmt: skip
N_INPUTS = [1, 2, 3, 128, 129]
SMOOTHS = [1, 3, 31]
#: status, model, scale, normalise, corrections
VARIANTS = list(itertools.product([True, False], repeat=5))
FULL = (True, True, True, True, True)
OUTPUTS = ("out", "kept", "filled", "fill_status", "mean_amplitude")
DTYPES = {"out": np.complex64, "kept": np.int32, "filled": np.int32, "fill_status": np.uint8,
          "mean_amplitude": np.float32}  # fmt: skip
MASK = 0x0F


@pytest.fixture(scope="module")
def context():
    from katsdpsigproc_amd import accel

    return accel.create_some_context(interactive=False)


@pytest.fixture(scope="module")
def command_queue(context):
    return context.create_command_queue()


@functools.lru_cache(maxsize=None)
def cached_case(seed, channels, n_inputs, max_gap, first=0):
    """{gains, status, model, scale}: never modified."""
    gains, status, model, scale, _ = gen.make_case(seed, channels, n_inputs, max_gap, first, MASK)
    case = {"gains": gains, "status": status, "model": model, "scale": scale}
    for array in case.values():
        array.flags.writeable = False
    return case


def inputs_of(case, variant):
    """The arguments of the host class after gains, None for what `variant` leaves out."""
    return [case[name] if wanted else None
            for name, wanted in zip(("status", "model", "scale"), variant)]  # fmt: skip


def outputs_of(variant):
    return [name for name in OUTPUTS if name != "mean_amplitude" or variant[3]]


@functools.lru_cache(maxsize=None)
def cached_want(key, smooth, variant):
    """What the host gives for cached_case(*key), by name. Never modified."""
    from katsdpsigproc_amd.rfi import host

    case = cached_case(*key)
    fn = host.InterpolateGainsHost(key[3], smooth, variant[3], MASK, variant[4])
    want = dict(zip(OUTPUTS, fn(case["gains"], *inputs_of(case, variant))))
    for array in want.values():
        if array is not None:
            array.flags.writeable = False
    return want


def hostile(padded_shape, dtype):
    """What the padding of an input holds: NaN, or bytes of 0xFF."""
    return poison_array(int(np.prod(padded_shape)), dtype).reshape(padded_shape)


def run_device(context, queue, case, max_gap, smooth, variant, pad=0, in_place=False):
    """The outputs of the operation by name. The padding of the inputs holds NaN or 0xFF; the
    outputs start out full of sentinel bytes (in place, `out` starts as gains in hostile
    padding). Afterwards every byte of padding is what it was, and so is every byte of the
    inputs that are not also the output."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import ingest

    with_status, with_model, with_scale, normalise, corrections = variant
    channels, n_inputs = case["gains"].shape
    template = ingest.InterpolateGainsTemplate(context, max_gap, smooth, normalise, with_status,
                                               MASK, with_model, with_scale, corrections)  # fmt: skip
    fn = template.instantiate(queue, channels, n_inputs)
    if pad:
        for k, (name, slot) in enumerate(fn.slots.items()):
            if in_place and name == "out":
                k = 0  # (the padding of gains)
            dim = slot.dimensions[-1]
            accel.Dimension(dim.size, min_padded_size=dim.size + (k + 1) * pad).link(dim)
    if in_place:
        fn.ensure_bound("gains")
        fn.bind(out=fn.buffer("gains"))
    fn.ensure_all_bound()
    uploaded = {}
    for name, wanted in zip(("gains", "status", "model", "scale"), (True,) + tuple(variant[:3])):
        if not wanted:
            continue
        d = fn.buffer(name)
        raw = hostile(d.padded_shape, d.dtype)
        raw[tuple(slice(n) for n in case[name].shape)] = case[name]
        queue.enqueue_write_buffer(d.buffer, raw)
        uploaded[name] = raw
    outputs = outputs_of(variant)
    before = {}
    for name in outputs:
        d = fn.buffer(name)
        before[name] = sentinel_array(d.padded_shape, d.dtype)
        if in_place and name == "out":
            before[name] = uploaded.pop("gains")
        else:
            queue.enqueue_write_buffer(d.buffer, before[name])
    fn()
    out = {}
    for name in outputs:
        d = fn.buffer(name)
        raw = np.empty(d.padded_shape, d.dtype)
        queue.enqueue_read_buffer(d.buffer, raw)
        data = tuple(slice(n) for n in d.shape)
        padding = np.ones(d.padded_shape, bool)
        padding[data] = False
        same = raw.view(np.uint8) == before[name].view(np.uint8)
        assert same[np.repeat(padding, d.dtype.itemsize, axis=-1)].all(), \
            f"wrote into the padding of {name}"  # fmt: skip
        out[name] = np.ascontiguousarray(raw[data])
    for name, sent in uploaded.items():
        d = fn.buffer(name)
        raw = np.empty(d.padded_shape, d.dtype)
        queue.enqueue_read_buffer(d.buffer, raw)
        assert (raw.view(np.uint8) == sent.view(np.uint8)).all(), f"{name} was modified"
    return out


def compare(context, queue, key, smooth=1, variant=FULL, pad=0, in_place=False):
    case = cached_case(*key)
    want = cached_want(key, smooth, variant)
    got = run_device(context, queue, case, key[3], smooth, variant, pad, in_place)
    assert list(got) == outputs_of(variant)
    for name, g in got.items():
        assert_same(want[name], g, f"{name} of {key}, smooth {smooth}, {variant}")
    return want


@pytest.mark.parametrize("step", STEPS, ids=lambda step: str(step[-2]))
def test_every_step_of_the_geometry(step, context, command_queue):
    """One channel below, at and one above every size at which the kernel changes path; the
    number of inputs, the kinds they start with, max_gap, smooth and the variant rotate."""
    for i, channels in enumerate(step):
        turn = i + len(step) * STEPS.index(step)
        n_inputs = (5, 16, 3)[i % 3] if channels <= 1025 else (3, 2, 4)[i % 3]
        key = (turn, channels, n_inputs, (8, 1, 70, 3)[turn % 4], 5 * turn)
        compare(context, command_queue, key, SMOOTHS[turn % 3], VARIANTS[(7 * turn) % 32])
        compare(context, command_queue, key, SMOOTHS[(turn + 1) % 3])


@pytest.mark.parametrize("n_inputs", N_INPUTS)
def test_inputs(n_inputs, context, command_queue):
    """One workgroup, odd strides, and more workgroups than compute units; with 128 and 129
    inputs every kind of data is there eight times."""
    seen = set()
    for channels, max_gap in ((37, 2), (300, 8), (1500, 5)):
        want = compare(context, command_queue, (n_inputs, channels, n_inputs, max_gap, n_inputs), 3)
        seen |= set(want["fill_status"].tolist())
    if n_inputs >= 128:
        assert seen == {0, 1, 2}


@pytest.mark.parametrize("first", range(0, len(gen.KINDS), 4))
def test_kinds(first, context, command_queue):
    """Four kinds of data at a time, each on its own among the inputs of a launch, at lengths on
    either side of every path of the kernel; the gaps of max_gap and max_gap + 1 channels lie
    across the wavefront's end at 64, the workgroup's at its thread count, and 4096."""
    for channels, max_gap in ((2, 1), (3, 0), (64, 3), (129, 8), (2048, 16), (5000, 100)):
        key = (first, channels, 4, max_gap, first)
        compare(context, command_queue, key)
        compare(context, command_queue, key, 3, (False, True, False, True, False))
        compare(context, command_queue, key, 1, (False, False, False, False, False))


@pytest.mark.parametrize("smooth", SMOOTHS)
def test_smooth(smooth, context, command_queue):
    """Windows that run over both ends of the band (5 and 20 channels at 31), windows whose
    only kept channel is their centre (`alternating` and `one_kept` at 3), and windows that
    reach into the next wavefront and the next round of the workgroup."""
    for channels in (5, 20, 100, 1030, 3000):
        key = (smooth, channels, len(gen.KINDS), 6, 0)
        compare(context, command_queue, key, smooth)
        compare(context, command_queue, key, smooth, (True, False, False, True, True))


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: "".join("ft"[x] for x in v))
def test_variants(variant, context, command_queue):
    compare(context, command_queue, (11, 150, 20, 4, 3), 3, variant)


@pytest.mark.parametrize("channels, n_inputs, pad", [(5, 3, 5), (130, 17, 1), (1100, 33, 16),
                                                      (4100, 5, 35)])  # fmt: skip
def test_in_place_and_padding(channels, n_inputs, pad, context, command_queue):
    """`out` bound to the buffer of `gains`, and rows padded beyond what the slots ask for, by
    a different amount for every slot (so the strides differ); run_device checks every byte of
    padding and of the inputs."""
    key = (pad, channels, n_inputs, 7, pad)
    for variant in VARIANTS[::5]:
        compare(context, command_queue, key, 3, variant, in_place=True)
        compare(context, command_queue, key, 3, variant, pad=pad)
        compare(context, command_queue, key, 1, variant, pad=pad, in_place=True)


@pytest.mark.parametrize("channels, n_inputs", [(6, 5), (3, 128), (70, 1), (300, 33), (1100, 3)])
@pytest.mark.parametrize("offset", [1, 3, 16])
def test_raw_abi_subviews(offset, channels, n_inputs, context, command_queue):
    """Sub-views: pointers `offset` elements into their allocations and an odd stride of its
    own for gains, model and out, with sentinels around every row; the variants rotate."""
    from katsdpsigproc_amd import _lib

    queue = command_queue
    views = CompactViews(context, queue)
    seed = 31 * offset + n_inputs
    variant = VARIANTS[seed % 32]
    with_status, with_model, with_scale, normalise, corrections = variant
    key = (seed, channels, n_inputs, 5, seed)
    case = cached_case(*key)
    want = cached_want(key, 3, variant)

    def view(name, data, stride, poison):
        return views(name, data.dtype, data, stride, offset, poison=poison)

    def blank(name, shape, stride):
        return view(name, sentinel_array(shape, DTYPES[name]), stride, False)

    d_in = {"gains": view("gains", case["gains"], (n_inputs + 4) | 1, True)}
    if with_status:
        d_in["status"] = view("status", case["status"][np.newaxis, :], channels, True)
    if with_model:
        d_in["model"] = view("model", case["model"], (n_inputs + 12) | 1, True)
    if with_scale:
        d_in["scale"] = view("scale", case["scale"][np.newaxis, :], n_inputs, True)
    d_out = {name: blank(name, (1, n_inputs), n_inputs) for name in outputs_of(variant)[1:]}
    d_out["out"] = blank("out", (channels, n_inputs), (n_inputs + 8) | 1)

    def pointer(views_by_name, name):
        return views_by_name[name][1] if name in views_by_name else None

    _lib.call("ksp_interpolate_gains", context.device.index, ctypes.c_void_p(queue.stream),
              pointer(d_in, "gains"), pointer(d_in, "status"), pointer(d_in, "model"),
              pointer(d_in, "scale"), pointer(d_out, "out"), pointer(d_out, "kept"),
              pointer(d_out, "filled"), pointer(d_out, "fill_status"),
              pointer(d_out, "mean_amplitude"), channels, n_inputs, d_in["gains"][0].stride,
              d_in["model"][0].stride if with_model else 0, d_out["out"][0].stride, 5, 3, MASK,
              int(corrections))  # fmt: skip
    for name, (d, _) in d_out.items():
        got = d.read(name)  # (asserts that nothing around the rows changed)
        assert_same(want[name], got if name == "out" else got[0], f"{name} at {offset}")
    for name, (d, _) in d_in.items():
        d.read(name)  # (asserts that nothing wrote to it)


def test_largest(context, command_queue):
    """The longest band with the widest window, and the shape of the time measurement."""
    compare(context, command_queue, (3, 16384, 5, 16384, 0), 31)
    compare(context, command_queue, (4, 4096, 128, 8, 0), 9, (True, True, False, True, True))


def test_host_from_device(context, command_queue):
    from katsdpsigproc_amd.rfi import ingest

    key = (21, 90, 18, 4, 0)
    case = cached_case(*key)
    for variant in VARIANTS[::3]:
        with_status, with_model, with_scale, normalise, corrections = variant
        template = ingest.InterpolateGainsTemplate(context, 4, 3, normalise, with_status, MASK,
                                                   with_model, with_scale, corrections)  # fmt: skip
        adapter = ingest.InterpolateGainsHostFromDevice(template, command_queue)
        got = adapter(case["gains"], *inputs_of(case, variant))
        want = cached_want(key, 3, variant)
        assert len(got) == 5 and (got[4] is not None) == normalise
        for name, g in zip(OUTPUTS, got):
            if g is not None:
                assert_same(want[name], g, f"{name} of {variant}")


#: the calibrator's flagged channels: 40 in runs of at most 8, one across the wavefront's end
FLAGGED_RUNS = ((10, 8), (60, 8), (100, 5), (126, 8), (180, 3), (220, 8))


def test_in_the_chain(context, command_queue):
    """A calibrator scan of 256 x 28 with a bandpass and a delay per input and 40 channels
    flagged, and a clean target scan with the same gains: solve -> fit_delays ->
    interpolate_gains -> apply_gains in one sequence against SolveGainsHost + FitDelaysHost +
    InterpolateGainsHost + ApplyGainsHost. The target comes out calibrated in every channel and
    no sample is flagged; with the solver's own corrections applied directly, every baseline
    is flagged in the 40 channels."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import host, ingest

    queue = command_queue
    channels, n_inputs, width, flag_value = 256, 8, 1e6, 0x40
    ants = np.ascontiguousarray(np.array(np.triu_indices(n_inputs, 1)).T, np.int32)
    baselines = len(ants)
    assert baselines == 28
    rs = np.random.RandomState(12)
    c = np.arange(channels)[:, np.newaxis]
    nus = rs.uniform(-0.02, 0.02, n_inputs)  # turns per channel
    nus[0] = 0.0
    ripple = 1 + 0.2 * np.cos(2 * np.pi * (c / rs.uniform(200, 400, n_inputs) + rs.uniform(size=n_inputs)))
    truth = ripple * np.exp(2j * np.pi * (c * nus + rs.uniform(size=n_inputs)))
    response = truth[:, ants[:, 0]] * np.conj(truth[:, ants[:, 1]])
    noise = 1e-3 * (rs.standard_normal(response.shape) + 1j * rs.standard_normal(response.shape))
    cal_vis = (response + noise).astype(np.complex64)
    cal_flags = np.zeros((channels, baselines), np.uint8)
    flagged = np.zeros(channels, bool)
    for start, length in FLAGGED_RUNS:
        flagged[start : start + length] = True
    assert flagged.sum() == 40
    cal_flags[flagged] = 1
    cal_vis[flagged] = 1e3  # (what interference leaves)
    sky = 2 + 0.5 * np.cos(np.arange(baselines))  # the target: not a unit source
    target_vis = (response * sky).astype(np.complex64)
    weights = np.ones((channels, baselines), np.float32)
    target_flags = np.zeros((channels, baselines), np.uint8)
    pairs = host.SolveGainsHost.pair_table(ants, n_inputs)

    solve = ingest.SolveGainsTemplate(context, max_iterations=60).instantiate(
        queue, channels, baselines, n_inputs)  # fmt: skip
    fit = ingest.FitDelaysTemplate(context, width).instantiate(queue, channels, n_inputs)
    interp = ingest.InterpolateGainsTemplate(context, 8, corrections=True).instantiate(
        queue, channels, n_inputs)  # fmt: skip
    apply_gains = ingest.ApplyGainsTemplate(context, flag_value=flag_value).instantiate(
        queue, channels, baselines, n_inputs)  # fmt: skip
    seq = accel.OperationSequence(
        queue, [("solve", solve), ("fit", fit), ("interp", interp), ("apply_gains", apply_gains)],
        compounds={"gains": ["solve:gains", "fit:gains", "interp:gains"],
                   "status": ["solve:status", "fit:status", "interp:status"],
                   "k": ["fit:model", "interp:model"],
                   "corr": ["interp:out", "apply_gains:gains"]})  # fmt: skip
    seq.ensure_all_bound()
    assert solve.buffer("gains") is fit.buffer("gains") is interp.buffer("gains")
    assert fit.buffer("model") is interp.buffer("model")
    assert interp.buffer("out") is apply_gains.buffer("gains")
    for name, value in (("solve:vis", cal_vis), ("solve:weights", weights),
                        ("solve:flags", cal_flags), ("solve:pairs", pairs),
                        ("apply_gains:vis", target_vis), ("apply_gains:weights", weights),
                        ("apply_gains:flags", target_flags), ("apply_gains:inputs", ants)):  # fmt: skip
        seq.buffer(name).set(queue, value)
    seq()

    gains, iterations, status = host.SolveGainsHost(max_iterations=60)(cal_vis, pairs, weights, cal_flags)
    assert np.isnan(gains[flagged]).all() and np.isfinite(gains[~flagged]).all()
    delays, phasors, amplitudes, fit_status, model = host.FitDelaysHost(width)(gains, status)
    corr, kept, filled, fill_status, _ = host.InterpolateGainsHost(8, corrections=True)(
        gains, status, model)  # fmt: skip
    out_vis, out_weights, out_flags = host.ApplyGainsHost(flag_value)(
        target_vis, corr, ants, weights, target_flags)  # fmt: skip
    for name, want in (("gains", gains), ("solve:iterations", iterations), ("status", status),
                       ("fit:delays", delays), ("fit:phasors", phasors),
                       ("fit:amplitudes", amplitudes), ("fit:fit_status", fit_status),
                       ("k", model), ("corr", corr), ("interp:kept", kept),
                       ("interp:filled", filled), ("interp:fill_status", fill_status),
                       ("apply_gains:out_vis", out_vis), ("apply_gains:out_weights", out_weights),
                       ("apply_gains:out_flags", out_flags)):  # fmt: skip
        assert_same(want, seq.buffer(name).get(queue), name)
    # every gap was filled, no sample is flagged, and the target is the sky in every channel
    assert not fit_status.any() and not fill_status.any()
    assert (kept == channels - 40).all() and (filled == 40).all()
    assert not seq.buffer("apply_gains:out_flags").get(queue).any()
    assert np.abs(out_vis / sky - 1).max() < 0.02

    # without the new step: the solver's own corrections, applied directly
    solve_direct = ingest.SolveGainsTemplate(context, max_iterations=60, corrections=True).instantiate(
        queue, channels, baselines, n_inputs)  # fmt: skip
    apply_direct = ingest.ApplyGainsTemplate(context, flag_value=flag_value).instantiate(
        queue, channels, baselines, n_inputs)  # fmt: skip
    direct = accel.OperationSequence(
        queue, [("solve", solve_direct), ("apply_gains", apply_direct)],
        compounds={"corr": ["solve:gains", "apply_gains:gains"]})
    direct.ensure_all_bound()
    for name, value in (("solve:vis", cal_vis), ("solve:weights", weights),
                        ("solve:flags", cal_flags), ("solve:pairs", pairs),
                        ("apply_gains:vis", target_vis), ("apply_gains:weights", weights),
                        ("apply_gains:flags", target_flags), ("apply_gains:inputs", ants)):  # fmt: skip
        direct.buffer(name).set(queue, value)
    direct()
    lost = direct.buffer("apply_gains:out_flags").get(queue)
    assert (lost[flagged] == flag_value).all() and not lost[~flagged].any()
