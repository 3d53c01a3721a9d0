"""Fitting per-input delays on the GPU (``rfi.ingest.FitDelaysTemplate``, ``ksp_fit_delays``):
every comparison is of bit patterns, of all five outputs, against ``rfi.host.FitDelaysHost``,
with nothing left out but the payload of a NaN that the host has as a NaN too."""

import ctypes
import functools
import itertools

import numpy as np
import pytest

from tests import inputs_fit_delays as gen
from tests.inputs_fit_delays import assert_same
from tests.subviews import CompactViews, poison_array, sentinel_array
from tests.test_gpu_prepare import LOST, N_AUTO

pytestmark = pytest.mark.gpu

# The sizes at which csrc/fit_delays.hip changes path. A transform of 4 runs in LDS alone; from 8
# on a thread does three stages on RUN = 8 elements in registers. The workgroup has n_fft / 8
# threads, at least 64 (up to n_fft = 512) and at most 1024 (from 8192 on, where a thread loads
# two runs at 16384). The sums of the refinement are thread-local for Cpad / threads = 1, 2, 4
# or 8 channels, cross wavefronts through LDS from Cpad = 128 on, and end in one wavefront.
N_FFTS = [4 << i for i in range(13)]
N_INPUTS = [1, 2, 3, 128, 129]
REFINES = [0, 1, 3, 8]
#: status, model, corrections
VARIANTS = list(itertools.product([True, False], repeat=3))
OUTPUTS = ("delays", "phasors", "amplitudes", "fit_status", "model")
DTYPES = {"delays": np.float64, "phasors": np.complex64, "amplitudes": np.float32,
          "fit_status": np.uint8, "model": np.complex64}  # fmt: skip
MASK = 0x0F


def channels_of(n_fft):
    return sorted({n_fft // 2, n_fft // 2 - 1, n_fft // 4 + 1, 1} - {0})


@pytest.fixture(scope="module")
def context():
    from katsdpsigproc_amd import accel

    return accel.create_some_context(interactive=False)


@pytest.fixture(scope="module")
def command_queue(context):
    return context.create_command_queue()


@functools.lru_cache(maxsize=None)
def cached_case(seed, channels, n_inputs, n_fft, first=0):
    """(gains, status, kinds): never modified."""
    gains, kinds, _ = gen.make_gains(seed, channels, n_inputs, n_fft, first)
    status = gen.make_status(seed + 1, channels, MASK)
    gains.flags.writeable = False
    status.flags.writeable = False
    return gains, status, kinds


@functools.lru_cache(maxsize=None)
def cached_want(key, n_fft, refine, with_status, corrections, width=-0.75e6):
    """What the host gives for cached_case(*key), by name. Never modified."""
    from katsdpsigproc_amd.rfi import host

    gains, status, _ = cached_case(*key)
    fn = host.FitDelaysHost(width, n_fft, refine, MASK, corrections)
    want = fn(gains, status if with_status else None)
    for array in want:
        array.flags.writeable = False
    return dict(zip(OUTPUTS, want))


def hostile(padded_shape, dtype):
    """What the padding of an input holds: NaN, or bytes of 0xFF."""
    return poison_array(int(np.prod(padded_shape)), dtype).reshape(padded_shape)


def run_device(context, queue, gains, status, n_fft, refine, variant, width=-0.75e6, pad=0):
    """The outputs of the operation by name. The padding of the inputs holds NaN or 0xFF; the
    outputs start out full of sentinel bytes. Afterwards every byte of padding is what it was,
    and so is every byte of the inputs."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import ingest

    with_status, with_model, corrections = variant
    channels, n_inputs = gains.shape
    template = ingest.FitDelaysTemplate(context, width, n_fft, refine, with_status, MASK,
                                        with_model, corrections)  # fmt: skip
    fn = template.instantiate(queue, channels, n_inputs)
    if pad:
        for k, (name, slot) in enumerate(fn.slots.items()):
            dim = slot.dimensions[-1]
            accel.Dimension(dim.size, min_padded_size=dim.size + (k + 1) * pad).link(dim)
    fn.ensure_all_bound()
    uploaded = {}
    for name, value in (("gains", gains), ("status", status)):
        if name == "status" and not with_status:
            continue
        d = fn.buffer(name)
        raw = hostile(d.padded_shape, d.dtype)
        raw[tuple(slice(n) for n in value.shape)] = value
        queue.enqueue_write_buffer(d.buffer, raw)
        uploaded[name] = raw
    outputs = [name for name in OUTPUTS if name != "model" or with_model]
    for name in outputs:
        d = fn.buffer(name)
        queue.enqueue_write_buffer(d.buffer, sentinel_array(d.padded_shape, d.dtype))
    fn()
    out = {}
    for name in outputs:
        d = fn.buffer(name)
        raw = np.empty(d.padded_shape, d.dtype)
        queue.enqueue_read_buffer(d.buffer, raw)
        data = tuple(slice(n) for n in d.shape)
        padding = np.ones(d.padded_shape, bool)
        padding[data] = False
        same = raw.view(np.uint8) == sentinel_array(d.padded_shape, d.dtype).view(np.uint8)
        assert same[np.repeat(padding, d.dtype.itemsize, axis=-1)].all(), \
            f"wrote into the padding of {name}"  # fmt: skip
        out[name] = np.ascontiguousarray(raw[data])
    for name, before in uploaded.items():
        d = fn.buffer(name)
        raw = np.empty(d.padded_shape, d.dtype)
        queue.enqueue_read_buffer(d.buffer, raw)
        assert (raw.view(np.uint8) == before.view(np.uint8)).all(), f"{name} was modified"
    return out


def compare(context, queue, key, n_fft, refine=3, variant=(True, True, False), pad=0):
    gains, status, _ = cached_case(*key)
    with_status, with_model, corrections = variant
    want = cached_want(key, n_fft, refine, with_status, corrections)
    got = run_device(context, queue, gains, status, n_fft, refine, variant, pad=pad)
    assert list(got) == [name for name in OUTPUTS if name != "model" or with_model]
    for name, g in got.items():
        assert_same(want[name], g, f"{name} of {key}, n_fft {n_fft}, refine {refine}, {variant}")
    return want


@pytest.mark.parametrize("n_fft", N_FFTS)
def test_every_transform_length(n_fft, context, command_queue):
    """Every n_fft with the longest band it takes, one channel fewer, a quarter plus one, and
    one channel; the number of inputs, the kinds they start with and the variant rotate."""
    for i, channels in enumerate(channels_of(n_fft)):
        n_inputs = N_INPUTS[(i + n_fft.bit_length()) % 5] if n_fft <= 1024 else (17, 3, 2, 1)[i]
        key = (n_fft + i, channels, n_inputs, n_fft, 5 * i)
        variant = VARIANTS[(i + n_fft.bit_length()) % 8]
        compare(context, command_queue, key, n_fft, REFINES[1 + i % 3], variant)


@pytest.mark.parametrize("n_inputs", N_INPUTS)
def test_inputs(n_inputs, context, command_queue):
    """One workgroup, odd strides, and more workgroups than compute units; with 128 and 129
    inputs every kind of data is there eight times."""
    for channels, n_fft in ((100, 256), (1000, 2048), (37, 1024)):
        want = compare(context, command_queue, (n_inputs, channels, n_inputs, n_fft, n_inputs), n_fft)
        if n_inputs >= 128:
            assert set(want["fit_status"].tolist()) >= {0, 1}


@pytest.mark.parametrize("first", range(0, len(gen.KINDS), 2))
def test_kinds(first, context, command_queue):
    """Two kinds of data at a time, each on its own among the inputs of a launch, at lengths
    on either side of every path of the kernel."""
    for channels, n_fft in ((2, 4), (3, 8), (64, 128), (129, 512), (2048, 4096), (3000, 16384)):
        key = (first, channels, 2, n_fft, first)
        compare(context, command_queue, key, n_fft)
        compare(context, command_queue, key, n_fft, 8, (False, True, True))


@pytest.mark.parametrize("refine", REFINES)
def test_refine(refine, context, command_queue):
    """Inputs of one launch stop early (a rejected step, no fit) and late."""
    for channels, n_fft in ((100, 256), (700, 2048)):
        want = compare(context, command_queue, (7, channels, 48, n_fft, 0), n_fft, refine)
        if refine:
            assert set(want["fit_status"].tolist()) >= {0, 1, 2}
        else:
            assert set(want["fit_status"].tolist()) == {0, 1}


@pytest.mark.parametrize("variant", VARIANTS)
def test_variants(variant, context, command_queue):
    for channels, n_fft in ((50, 128), (513, 2048)):
        compare(context, command_queue, (11, channels, 20, n_fft, 3), n_fft, 3, variant)


@pytest.mark.parametrize("channels, n_inputs, n_fft, pad", [
    (5, 3, 16, 5), (33, 17, 128, 1), (200, 64, 512, 16), (1025, 5, 4096, 35), (4096, 2, 16384, 3)])  # fmt: skip
def test_padding(channels, n_inputs, n_fft, pad, context, command_queue):
    """Rows padded beyond what the slots ask for, by a different amount for every slot (so the
    strides differ); run_device checks every byte of padding and of the inputs."""
    key = (pad, channels, n_inputs, n_fft, pad)
    for variant in VARIANTS[::3]:
        compare(context, command_queue, key, n_fft, 3, variant, pad)


@pytest.mark.parametrize("channels, n_inputs, n_fft", [(6, 5, 16), (3, 128, 8), (70, 1, 256),
                                                        (300, 33, 1024), (2, 3, 4)])  # fmt: skip
@pytest.mark.parametrize("offset", [1, 3, 16])
def test_raw_abi_subviews(offset, channels, n_inputs, n_fft, context, command_queue):
    """Sub-views: pointers `offset` elements into their allocations and an odd stride of its own
    for gains and model; the variants rotate."""
    check_raw_abi(offset, channels, n_inputs, n_fft, context, command_queue)


def check_raw_abi(offset, channels, n_inputs, n_fft, context, command_queue, views=None,
                  variant=None):
    """`views` makes the arrays (tests/subviews.py: CompactViews unless given) and may choose
    other strides of the same kind; `variant` instead of the one that is due by rotation."""
    from katsdpsigproc_amd import _lib

    queue = command_queue
    views = views or CompactViews(context, queue)
    seed = 31 * offset + n_inputs
    with_status, with_model, corrections = variant or VARIANTS[seed % 8]
    key = (seed, channels, n_inputs, n_fft, seed)
    gains, status, _ = cached_case(*key)
    want = cached_want(key, n_fft, 2, with_status, corrections, 1e5)

    def view(name, data, stride, poison):
        return views(name, data.dtype, data, stride, offset, poison=poison)

    def blank(name, shape):
        return view(name, sentinel_array(shape, DTYPES[name]), shape[1] if shape[0] == 1 else
                    (n_inputs + 8) | 1, False)  # fmt: skip

    d_gains = view("gains", gains, (n_inputs + 4) | 1, True)
    d_status = view("status", status[np.newaxis, :], channels, True) if with_status else None
    d_out = {name: blank(name, (1, n_inputs)) for name in OUTPUTS[:4]}
    if with_model:
        d_out["model"] = blank("model", (channels, n_inputs))
    _lib.call("ksp_fit_delays", context.device.index, ctypes.c_void_p(queue.stream),
              d_gains[1], d_status[1] if with_status else None, d_out["delays"][1],
              d_out["phasors"][1], d_out["amplitudes"][1], d_out["fit_status"][1],
              d_out["model"][1] if with_model else None, channels, n_inputs, d_gains[0].stride,
              d_out["model"][0].stride if with_model else 0, n_fft, 2, MASK, int(corrections),
              1e5)  # fmt: skip
    for name, (d, _) in d_out.items():
        got = d.read(name)  # (asserts that nothing around the rows changed)
        assert_same(want[name], got if name == "model" else got[0], f"{name} at {offset}")
    d_gains[0].read("gains")  # (asserts that nothing wrote to it)
    if with_status:
        d_status[0].read("status")


def test_largest(context, command_queue):
    """The largest transform with the longest band, and the shape of the time measurement."""
    compare(context, command_queue, (3, 8192, 5, 16384, 0), 16384)
    compare(context, command_queue, (4, 4096, 128, 16384, 0), 16384)


def test_host_from_device(context, command_queue):
    from katsdpsigproc_amd.rfi import ingest

    key = (21, 90, 18, 512, 0)
    gains, status, _ = cached_case(*key)
    for variant in VARIANTS:
        with_status, with_model, corrections = variant
        template = ingest.FitDelaysTemplate(context, -0.75e6, 512, 3, with_status, MASK,
                                            with_model, corrections)  # fmt: skip
        adapter = ingest.FitDelaysHostFromDevice(template, command_queue)
        got = adapter(gains, status if with_status else None)
        want = cached_want(key, 512, 3, with_status, corrections)
        assert len(got) == 5 and (got[4] is not None) == with_model
        for name, g in zip(OUTPUTS, got):
            if g is not None:
                assert_same(want[name], g, f"{name} of {variant}")
    # the default length: four times the band, rounded up
    template = ingest.FitDelaysTemplate(context, 1e6, status=False)
    from katsdpsigproc_amd.rfi import host

    got = ingest.FitDelaysHostFromDevice(template, command_queue)(gains)
    for name, w, g in zip(OUTPUTS, host.FitDelaysHost(1e6)(gains), got):
        assert_same(w, g, name)


def delay_dump(seed, in_baselines, source, ants, truth, unit):
    """int32 (channels, in_baselines, 2): ``g_a conj(g_b)`` of a unit point source for the
    per-channel gains `truth` (channels, n_inputs) plus 1 % noise, in units of 1 / `unit`, at
    the input baselines `source` names; autocorrelations of about 8 in the first N_AUTO; noise
    everywhere else; about 3 % lost samples."""
    rs = np.random.RandomState(seed)
    shape = (len(truth), in_baselines)
    noise = 0.01 * (rs.standard_normal(shape) + 1j * rs.standard_normal(shape))
    vis = noise.copy()
    vis[:, source] += truth[:, ants[:, 0]] * np.conj(truth[:, ants[:, 1]])
    vis[:, :N_AUTO] = 8 + noise[:, :N_AUTO].real
    vis_in = np.empty(shape + (2,), np.int32)
    vis_in[..., 0] = np.rint(vis.real * unit)
    vis_in[..., 1] = np.rint(vis.imag * unit)
    lost = rs.random_sample(shape) < 0.03
    lost[:, :N_AUTO] = False
    vis_in[lost, 0] = LOST
    return vis_in


def test_in_the_chain(context, command_queue):
    """Three dumps of 64 x 40 model data with per-input delays through prepare -> fused flagger
    -> accumulate -> finalise -> solve -> fit_delays -> apply_gains in one sequence, against
    PrepareHost + FlaggerHost + AveragerHost + SolveGainsHost + FitDelaysHost + ApplyGainsHost;
    apply_gains multiplies by the fitted phasors, and the calibrated cross-correlations are the
    unit source."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import device, host, ingest

    queue = command_queue
    channels, in_baselines, cf, n_inputs = 64, 60, 4, 9
    rows = channels // cf
    width = 1e6
    rs = np.random.RandomState(9)
    cross = np.array(np.triu_indices(n_inputs, 1)).T
    cross = cross[rs.permutation(len(cross))]
    swap = rs.random_sample(len(cross)) < 0.5
    cross[swap] = cross[swap][:, ::-1]
    autos = np.repeat(np.arange(4)[:, np.newaxis], 2, axis=1)
    ants = np.ascontiguousarray(np.concatenate([cross[:20], autos, cross[20:]]), np.int32)
    baselines = len(ants)  # 36 cross-correlations and 4 autocorrelations
    full = device.BackgroundFlags.FULL
    unit = 2.0**17
    scale, lost_flag, weight_scale = 1 / unit, 0x08, 64.0
    prepare = ingest.PrepareTemplate(context, scale, lost_flag, False, True, weight_scale).instantiate(
        queue, channels, baselines, in_baselines)  # fmt: skip
    flagger = device.FlaggerDeviceTemplate(
        device.BackgroundMedianFilterDeviceTemplate(context, 13, use_flags=full),
        device.NoiseEstMADTDeviceTemplate(context, channels),
        device.ThresholdSumDeviceTemplate(context),
        fused=True, tuning={"vis_pad": 0},
    ).instantiate(queue, channels, baselines, threshold_args={"n_sigma": 11.0})
    accumulate = device.AccumulateTemplate(context, use_weights=True, input_flags=full).instantiate(
        queue, channels, baselines)  # fmt: skip
    finalise = device.FinaliseTemplate(context, channel_factor=cf).instantiate(
        queue, channels, baselines)  # fmt: skip
    solve = ingest.SolveGainsTemplate(context, max_iterations=60).instantiate(
        queue, rows, baselines, n_inputs)  # fmt: skip
    fit = ingest.FitDelaysTemplate(context, cf * width, corrections=True).instantiate(
        queue, rows, n_inputs)  # fmt: skip
    apply_gains = ingest.ApplyGainsTemplate(context, flag_value=0x40).instantiate(
        queue, rows, baselines, n_inputs)  # fmt: skip
    acc = ("acc_vis", "acc_weights", "acc_flags")
    compounds = {
        "vis": ["prepare:vis", "flagger:vis", "accumulate:vis"],
        "input_flags": ["prepare:input_flags", "flagger:input_flags", "accumulate:input_flags"],
        "weights": ["prepare:weights", "accumulate:weights"],
        "flags": ["flagger:flags", "accumulate:flags"],
        "avg_vis": ["finalise:vis", "solve:vis", "apply_gains:vis"],
        "avg_weights": ["finalise:weights", "solve:weights", "apply_gains:weights"],
        "avg_flags": ["finalise:flags", "solve:flags", "apply_gains:flags"],
        "gains": ["solve:gains", "fit:gains"],
        "status": ["solve:status", "fit:status"],
        "corrections": ["fit:model", "apply_gains:gains"],
    }
    compounds.update({name: ["accumulate:" + name, "finalise:" + name] for name in acc})
    seq = accel.OperationSequence(
        queue, [("prepare", prepare), ("flagger", flagger), ("accumulate", accumulate),
                ("finalise", finalise), ("solve", solve), ("fit", fit),
                ("apply_gains", apply_gains)],
        compounds=compounds)  # fmt: skip
    for name in device.FusedFlaggerDevice._OPTIONAL:
        del seq.slots["flagger:" + name]
    seq.ensure_all_bound()
    assert solve.buffer("gains") is fit.buffer("gains")
    assert solve.buffer("status") is fit.buffer("status")
    assert fit.buffer("model") is apply_gains.buffer("gains")
    for name in acc:
        seq.buffer(name).zero(queue)
    source = (N_AUTO + rs.permutation(in_baselines - N_AUTO)[:baselines]).astype(np.int32)
    auto_source = rs.randint(0, N_AUTO, (baselines, 2)).astype(np.int32)
    # delays of up to 10 ns over a band of 64 MHz: at most 0.01 turns per unaveraged channel
    true_delays = rs.uniform(-1e-8, 1e-8, n_inputs)
    true_delays[0] = 0.0
    phases = rs.uniform(-np.pi, np.pi, n_inputs)
    fine = np.arange(channels)[:, np.newaxis] * width
    truth = np.exp(1j * (phases + 2 * np.pi * fine * true_delays))
    pairs = host.SolveGainsHost.pair_table(ants, n_inputs)
    seq.buffer("prepare:source").set(queue, source)
    seq.buffer("prepare:auto_source").set(queue, auto_source)
    seq.buffer("solve:pairs").set(queue, pairs)
    seq.buffer("apply_gains:inputs").set(queue, ants)
    prepare_host = host.PrepareHost(scale, lost_flag, weight_scale)
    flagger_host = host.FlaggerHost(host.BackgroundMedianFilterHost(13), host.NoiseEstMADHost(),
                                    host.ThresholdSumHost(11.0))  # fmt: skip
    averager = host.AveragerHost(channels, baselines, cf, full)
    solve_host = host.SolveGainsHost(max_iterations=60)
    fit_host = host.FitDelaysHost(cf * width, corrections=True)
    apply_host = host.ApplyGainsHost(0x40)

    def host_dump(vis_in):
        vis, input_flags, weights = prepare_host(vis_in, source, None, auto_source)
        flags = flagger_host(vis, input_flags)
        averager.add(vis, flags, weights, input_flags=input_flags)

    def check_outputs():
        vis, weights, flags = averager.finalise()
        gains, iterations, status = solve_host(vis, pairs, weights, flags)
        delays, phasors, amplitudes, fit_status, model = fit_host(gains, status)
        cal_vis, cal_weights, cal_flags = apply_host(vis, model, ants, weights, flags)
        for name, w in (("avg_vis", vis), ("avg_weights", weights), ("avg_flags", flags),
                        ("gains", gains), ("solve:iterations", iterations), ("status", status),
                        ("fit:delays", delays), ("fit:phasors", phasors),
                        ("fit:amplitudes", amplitudes), ("fit:fit_status", fit_status),
                        ("corrections", model), ("apply_gains:out_vis", cal_vis),
                        ("apply_gains:out_weights", cal_weights),
                        ("apply_gains:out_flags", cal_flags)):  # fmt: skip
            assert_same(w, seq.buffer(name).get(queue), name)
        return delays, fit_status, cal_vis, cal_flags

    for d in range(3):
        vis_in = delay_dump(20 + d, in_baselines, source, ants, truth, unit)
        seq.buffer("prepare:vis_in").set(queue, vis_in)
        prepare()
        flagger()
        accumulate()
        host_dump(vis_in)
    finalise()
    solve()
    fit()
    apply_gains()
    delays, fit_status, cal_vis, cal_flags = check_outputs()
    # the fit is the model's: every input fitted, the delays those of the dumps relative to
    # the reference input, and the calibrated cross-correlations are 1
    assert not fit_status.any()
    assert np.abs(delays - true_delays).max() < 2e-10
    is_cross = ants[:, 0] != ants[:, 1]
    good = (cal_flags == 0) & is_cross[np.newaxis, :]
    assert good.mean() > 0.7 and np.abs(cal_vis[good] - 1).max() < 0.1
    # and once more through the sequence as a whole
    vis_in = delay_dump(40, in_baselines, source, ants, truth, unit)
    seq.buffer("prepare:vis_in").set(queue, vis_in)
    seq()
    host_dump(vis_in)
    check_outputs()
