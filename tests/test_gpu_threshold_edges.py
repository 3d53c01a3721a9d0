"""Thresholds on their limit, on the GPU, bit for bit against the CPU oracle.

The fused kernels decide a SumThreshold window, or a sample of the simple threshold, from float32
deviations with an error bound and go back to exact float64 deviations for what the bound leaves
undecided. Every planted window of ``tests/inputs_threshold_edges.py`` is undecided, and the
float32 values alone decide it wrongly (``tests/test_threshold_edges.py`` asserts that, and that
the oracle used here equals ``rfi.host`` and the reference on these inputs). The paths: the
4-baseline kernel (lanes of 16 channels and the direct window loop at 320 channels, width 13 and
up to 4 windows; lanes of 64 and ``threshold_wide`` otherwise), the ring kernel, the long-band
kernels, each with ``ksp_flagger_fused_last_path`` asserted.

The stand-alone launchers and the five-kernel sequence take float32 deviations, so there the limit
is equality itself: ``equality_case`` plants windows whose sum *is* ``w * thr_k`` and windows one
float32 step above it.
"""

import numpy as np
import pytest

from tests import inputs_threshold_edges as edges

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def context():
    from katsdpsigproc_amd import accel

    return accel.create_some_context(interactive=False)


@pytest.fixture(scope="module")
def command_queue(context):
    return context.create_command_queue()


@pytest.fixture(scope="module")
def oracle():
    from oracle import rfi_oracle

    rfi_oracle.set_threads(min(rfi_oracle.max_threads(), 16))
    yield rfi_oracle
    rfi_oracle.set_threads(1)


# ------------------------------------------------------------------ fused kernels
def fused_template(context, case, keep_deviations):
    from katsdpsigproc_amd.rfi import device

    mode = device.BackgroundFlags.NONE if case.in_flags is None else device.BackgroundFlags.CHANNEL
    bg = device.BackgroundMedianFilterDeviceTemplate(context, case.width, case.amplitudes, mode)
    ne = device.NoiseEstMADTDeviceTemplate(context, 10240)
    if case.kind == "sum":
        th = device.ThresholdSumDeviceTemplate(context, case.n_windows, tuning={"wgs": 256, "vt": 0})
    else:
        th = device.ThresholdSimpleDeviceTemplate(context, False)
    return device.FlaggerDeviceTemplate(bg, ne, th, keep_deviations=keep_deviations)


def threshold_args(case):
    args = {"n_sigma": case.n_sigma}
    if case.kind == "sum":
        args["threshold_falloff"] = case.threshold_falloff
    return args


def run_fused(context, queue, oracle, case, ring_mode, expected_path, launches=1):
    """`case` through the fused flagger: flags, noise (and deviations where kept) equal the
    oracle's, the flags at every planted window among them, by the kernels of `expected_path`."""
    from katsdpsigproc_amd import _lib
    from katsdpsigproc_amd.rfi import device

    ref_flags, ref_noise, ref_dev = oracle.flagger_full(
        case.vis, case.in_flags, width=case.width, amplitudes=case.amplitudes, threshold=case.kind,
        n_sigma=case.n_sigma, n_windows=case.n_windows, threshold_falloff=case.threshold_falloff,
        want_deviations=True)  # fmt: skip
    template = fused_template(context, case, case.keep_deviations)
    fn = template.instantiate(queue, *case.vis.shape, threshold_args=threshold_args(case))
    assert isinstance(fn, device.FusedFlaggerDevice)
    fn.ensure_all_bound()
    fn.buffer("vis").set(queue, case.vis)
    if case.in_flags is not None:
        fn.buffer("input_flags").set(queue, case.in_flags)
    for _ in range(launches):
        fn.buffer("flags").set(queue, np.full(case.vis.shape, 255, np.uint8))
        with _lib.fused_ring_mode(ring_mode):
            fn()
        path = _lib.call("ksp_flagger_fused_last_path")
        assert path == expected_path, f"last path = {path}, expected {expected_path}"
        flags = fn.buffer("flags").get(queue)
        np.testing.assert_array_equal(ref_noise.astype(np.float32), fn.buffer("noise").get(queue))
        if case.keep_deviations:
            np.testing.assert_array_equal(ref_dev.astype(np.float32),
                                          fn.buffer("deviations").get(queue))  # fmt: skip
        for b, c, w in case.planted:  # (named first: a failure says which window)
            np.testing.assert_array_equal(
                ref_flags[c : c + w, b], flags[c : c + w, b],
                err_msg=f"{case.name}: window of {w} at channel {c} of baseline {b}")
        np.testing.assert_array_equal(ref_flags, flags)


@pytest.mark.parametrize("name", edges.names("fused4"))
def test_four_baseline_kernel(name, context, command_queue, oracle):
    from katsdpsigproc_amd import _lib

    run_fused(context, command_queue, oracle, edges.by_name(name), -1, _lib.FUSED_PATH_STRIP)


@pytest.mark.parametrize("name", edges.names("ring"))
def test_ring_kernel(name, context, command_queue, oracle):
    """Forced, and launched twice: the second launch finds the scheduling counters as the first
    left them. 12 baselines are a ring strip of 8 and a remainder for the 4-baseline kernel."""
    from katsdpsigproc_amd import _lib

    case = edges.by_name(name)
    path = _lib.FUSED_PATH_RING | (_lib.FUSED_PATH_STRIP if case.vis.shape[1] % 8 else 0)
    run_fused(context, command_queue, oracle, case, 1, path, launches=2)


@pytest.mark.parametrize("name", edges.names("long"))
def test_long_band_kernels(name, context, command_queue, oracle):
    from katsdpsigproc_amd import _lib

    run_fused(context, command_queue, oracle, edges.by_name(name), -1, _lib.FUSED_PATH_LONG)


@pytest.mark.parametrize("args", edges.BAND_END, ids=lambda a: f"{a[0]}_{a[1][0]}x{a[1][1]}_w{a[2]}")
def test_window_past_the_band_end(args, context, command_queue, oracle):
    """The last ``w - 1`` channels alone exceed the limit, the last full window does not: a window
    that starts one channel too far, padded with the zero beyond the band, must not count."""
    from katsdpsigproc_amd import _lib

    case = edges.band_end_case(*args)
    baselines = case.vis.shape[1]
    ring_mode, path, launches = {
        "fused4": (-1, _lib.FUSED_PATH_STRIP, 1),
        "ring": (1, _lib.FUSED_PATH_RING | (_lib.FUSED_PATH_STRIP if baselines % 8 else 0), 2),
        "long": (-1, _lib.FUSED_PATH_LONG, 1),
    }[case.path]
    run_fused(context, command_queue, oracle, case, ring_mode, path, launches)


# ------------------------------------------------------------------ float32 deviations: equality
SCENARIOS = ("equal", "raised", "replaced_equal", "replaced_raised")


def thresholds(noise, n_sigma, n_windows, falloff=1.2):
    """thr_k per baseline as ``ThresholdSumHost`` computes them from float32 noise: float32 all
    the way (NumPy takes the Python floats as float32)."""
    noise = np.asarray(noise, np.float32)
    t1 = n_sigma * noise
    assert t1.dtype == np.float32
    return np.stack([(t1 * pow(falloff, -k)).astype(np.float32) for k in range(n_windows)])


def plant(dev, expected, thr, b, c, k, scenario, lift):
    """One window of ``w = 2**k`` channels at channel `c` of baseline `b`:

    * ``equal``: every sample is ``thr_k``, the sum is the limit, nothing is flagged;
    * ``raised``: the same with sample `lift` one float32 step up: all `w` are flagged;
    * ``replaced_equal`` / ``replaced_raised``: ``w - 1`` samples of ``100 thr_0``, which window 1
      flags and which then count as exactly ``thr_k``, and a last sample at ``thr_k`` (not
      flagged) or one step above it (flagged).

    Smaller windows do not fire on these (``thr`` falls with k), larger ones hold quiet samples
    that are not positive (and flagged samples count as their own, smaller, threshold)."""
    w = 1 << k
    t = thr[k, b]
    up = np.nextafter(t, np.float32(np.inf))
    assert up > t > 0
    if scenario in ("equal", "raised"):
        dev[c : c + w, b] = t
        if scenario == "raised":
            dev[c + lift % w, b] = up
            expected[c : c + w, b] = 1
    else:
        dev[c : c + w - 1, b] = thr[0, b] * np.float32(100)
        expected[c : c + w - 1, b] = 1
        dev[c + w - 1, b] = up if scenario == "replaced_raised" else t
        expected[c + w - 1, b] = scenario == "replaced_raised"


def equality_case(channels, baselines, n_windows, boundaries, n_sigma=11.0, seed=1):
    """Channel-major float32 deviations, float32 noise and the flags they must give. Baseline b
    holds one scenario at one window size (all of them in turn), inside a chunk and across every
    boundary of `boundaries`; two more kinds of baseline hold nothing above ``thr_min``, or
    ``thr_min (1 - 2**-21)``, which the fast reject must leave without flags, and the baselines
    whose only window is one step above ``thr_min`` are what it must not reject."""
    rs = np.random.RandomState(seed)
    noise = (0.9 + 0.2 * rs.random_sample(baselines)).astype(np.float32)
    thr = thresholds(noise, n_sigma, n_windows)
    # quiet samples: not positive, so that no window gains from them
    dev = (-0.5 * rs.random_sample((channels, baselines))).astype(np.float32)
    expected = np.zeros((channels, baselines), np.uint8)
    combos = [(k, s) for k in range(n_windows) for s in SCENARIOS] + [(None, "min"), (None, "below")]
    for b in range(baselines):
        k, scenario = combos[b % len(combos)]
        if k is None:
            t = thr[n_windows - 1, b]
            value = t if scenario == "min" else np.float32(float(t) * (1 - 2.0**-21))
            assert scenario == "min" or value < t
            dev[100 + b, b] = value
            continue
        w = 1 << k
        firsts = [100 + b]
        for boundary in boundaries:
            j = 1 + b % (w - 1) if w > 1 else 1
            firsts.append(min(boundary - j, channels - w))
        assert all(y - x >= 256 for x, y in zip(firsts, firsts[1:]))  # (no window sees two)
        for i, c in enumerate(firsts):
            plant(dev, expected, thr, b, c, k, scenario, lift=b + i)
    return dev, noise, expected


def cm_core(channels, baselines, n_windows):
    """Channels per segment of the channel-major launcher (its geometry, restated)."""
    edge = 2**n_windows - n_windows - 1
    want = -(-8192 // -(-baselines // 64))
    return min(channels, max(-(-channels // want), 4 * edge, 64))


def run_threshold(context, queue, dev, noise, n_sigma, n_windows, tuning=None, transposed=True):
    from katsdpsigproc_amd.rfi import device

    channels, baselines = dev.shape
    template = device.ThresholdSumDeviceTemplate(context, n_windows, 1, tuning, transposed=transposed)
    fn = template.instantiate(queue, channels, baselines, n_sigma)
    fn.ensure_all_bound()
    fn.buffer("deviations").set(queue, np.ascontiguousarray(dev.T) if transposed else dev)
    fn.buffer("noise").set(queue, noise)
    fn.buffer("flags").set(queue, np.full(fn.buffer("flags").shape, 255, np.uint8))
    fn()
    flags = fn.buffer("flags").get(queue)
    return np.ascontiguousarray(flags.T) if transposed else flags


@pytest.mark.parametrize("n_windows", [4, 8])
@pytest.mark.parametrize("channels", [4100, 9001])
def test_sum_launchers_at_equality(channels, n_windows, context, command_queue, oracle):
    """``ksp_threshold_sum`` with every vt (chunks of 2048, 4096 and 8192 channels, so windows
    across the halo of two chunks) and ``ksp_threshold_sum_cm`` (windows across a segment boundary,
    65 baselines: the last lane of a wavefront and the first of the next)."""
    baselines = 65
    core = cm_core(channels, baselines, n_windows)
    boundaries = sorted({b for b in (core, 2048, 4096, 8192) if 300 < b < channels})
    dev, noise, expected = equality_case(channels, baselines, n_windows, boundaries)
    ref = oracle.ThresholdSumHost(11.0, n_windows)(dev, noise)
    np.testing.assert_array_equal(expected, ref)  # (the construction is what it says)
    assert expected[:, [63, 64]].any()
    for vt in (8, 16, 32):
        out = run_threshold(context, command_queue, dev, noise, 11.0, n_windows,
                            {"wgs": 256, "vt": vt})  # fmt: skip
        np.testing.assert_array_equal(ref, out, err_msg=f"vt={vt}")
    out = run_threshold(context, command_queue, dev, noise, 11.0, n_windows, transposed=False)
    np.testing.assert_array_equal(ref, out, err_msg="channel-major")


def test_simple_launcher_at_equality(context, command_queue, oracle):
    """``deviation > n_sigma * noise`` in float32: a sample at the limit is not flagged, one step
    above it is, in both layouts."""
    from katsdpsigproc_amd.rfi import device

    rs = np.random.RandomState(2)
    channels, baselines = 300, 65
    noise = (0.9 + 0.2 * rs.random_sample(baselines)).astype(np.float32)
    limit = thresholds(noise, 11.0, 1)[0]
    dev = (-0.5 * rs.random_sample((channels, baselines))).astype(np.float32)
    expected = np.zeros(dev.shape, np.uint8)
    for b in range(baselines):
        dev[3 * b, b] = limit[b]
        dev[3 * b + 1, b] = np.nextafter(limit[b], np.float32(np.inf))
        dev[3 * b + 2, b] = np.nextafter(limit[b], np.float32(-np.inf))
        expected[3 * b + 1, b] = 1
    ref = oracle.ThresholdSimpleHost(11.0)(dev, noise)
    np.testing.assert_array_equal(expected, ref)
    for transposed in (False, True):
        template = device.ThresholdSimpleDeviceTemplate(context, transposed)
        fn = template.instantiate(command_queue, channels, baselines, 11.0)
        fn.ensure_all_bound()
        fn.buffer("deviations").set(command_queue, np.ascontiguousarray(dev.T) if transposed else dev)
        fn.buffer("noise").set(command_queue, noise)
        fn()
        out = fn.buffer("flags").get(command_queue)
        np.testing.assert_array_equal(ref, out.T if transposed else out)


@pytest.mark.parametrize("transposed", [True, False])
def test_sequence_at_equality(transposed, context, command_queue, oracle):
    """The five-kernel sequence (width 33, which the fused kernel refuses) on 320 x 5 amplitudes
    whose deviations are the amplitudes themselves: quiet channels 0 or -0.25 (every median 0,
    the noise 1.4826 * 0.25 in float32), and every scenario of ``plant`` at every window size.
    Its deviations are float32 by definition: the reference is the oracle's stages chained
    through float32."""
    from katsdpsigproc_amd.rfi import device

    channels, baselines, width, n_windows, n_sigma = 320, 5, 33, 4, 11.0
    amp = np.zeros((channels, baselines), np.float32)
    amp[::5] = -0.25
    noise32 = oracle.NoiseEstMADHost()(amp).astype(np.float32)
    thr = thresholds(noise32, n_sigma, n_windows)
    expected = np.zeros(amp.shape, np.uint8)
    combos = [(k, s) for k in range(n_windows) for s in SCENARIOS]
    for i, (k, scenario) in enumerate(combos):
        b, slot = i % baselines, i // baselines
        c = (0, 77, 160, 320 - (1 << k))[slot]  # (the band's first and last channels among them)
        amp[c : c + 8, b] = 0
        plant(amp, expected, thr, b, c, k, scenario, lift=i)

    bg = device.BackgroundMedianFilterDeviceTemplate(context, width, True)
    ne = device.NoiseEstMADTDeviceTemplate(context, 10240)
    th = device.ThresholdSumDeviceTemplate(context, n_windows, tuning={"wgs": 256, "vt": 0},
                                           transposed=transposed)  # fmt: skip
    template = device.FlaggerDeviceTemplate(bg, ne, th)
    assert not template.fusable(channels)
    fn = template.instantiate(command_queue, channels, baselines, threshold_args={"n_sigma": n_sigma})
    assert isinstance(fn, device.FlaggerDevice)
    fn.ensure_all_bound()
    fn.buffer("vis").set(command_queue, amp)
    fn()

    dev32 = oracle.BackgroundMedianFilterHost(width, True)(amp).astype(np.float32)
    np.testing.assert_array_equal(amp, dev32)  # (the premise: every median is 0)
    np.testing.assert_array_equal(noise32, oracle.NoiseEstMADHost()(dev32).astype(np.float32))
    flags = oracle.ThresholdSumHost(n_sigma, n_windows)(dev32, noise32)
    np.testing.assert_array_equal(expected, flags)
    np.testing.assert_array_equal(dev32, fn.buffer("deviations").get(command_queue))
    np.testing.assert_array_equal(noise32, fn.buffer("noise").get(command_queue))
    np.testing.assert_array_equal(flags, fn.buffer("flags").get(command_queue))
