"""SumThreshold on channel-major deviations on the GPU: every case bit for bit against the
CPU oracle's ThresholdSumHost and against ``ksp_threshold_sum`` on the transposed array,
and the kernel-per-stage flagger built on it against the oracle's stages."""

import numpy as np
import pytest

from tests import inputs

pytestmark = pytest.mark.gpu

CHANNELS = [1, 7, 255, 256, 4096, 8191]
BASELINES = [1, 63, 64, 65]


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


def run_cm(context, queue, dev, noise, n_sigma, n_windows, flag_value=1, pad=0):
    """Flags of channel-major `dev` through ``transposed=False``, rows padded by `pad`."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import device

    channels, baselines = dev.shape
    template = device.ThresholdSumDeviceTemplate(context, n_windows, flag_value, transposed=False)
    fn = template.instantiate(queue, channels, baselines, n_sigma)
    if pad:
        dim = fn.slots["deviations"].dimensions[1]
        accel.Dimension(dim.size, min_padded_size=dim.size + pad).link(dim)
    fn.ensure_all_bound()
    assert fn.buffer("deviations").padded_shape[1] >= baselines + pad
    fn.buffer("deviations").set(queue, dev)
    fn.buffer("noise").set(queue, noise)
    # poison the flags, padding included: every written byte must be the kernel's
    flags = fn.buffer("flags")
    queue.enqueue_write_buffer(flags.buffer, np.full(flags.padded_shape, 0xAB, np.uint8))
    fn()
    raw = np.empty(flags.padded_shape, np.uint8)
    queue.enqueue_read_buffer(flags.buffer, raw)
    assert np.all(raw[:, baselines:] == 0xAB), "wrote into the row padding"
    return np.ascontiguousarray(raw[:, :baselines])


def run_bm(context, queue, dev, noise, n_sigma, n_windows, flag_value=1):
    """The same through the baseline-major kernel on the transposed array."""
    from katsdpsigproc_amd.rfi import device

    channels, baselines = dev.shape
    template = device.ThresholdSumDeviceTemplate(context, n_windows, flag_value, {"vt": 0})
    fn = template.instantiate(queue, channels, baselines, n_sigma)
    fn.ensure_all_bound()
    fn.buffer("deviations").set(queue, np.ascontiguousarray(dev.T))
    fn.buffer("noise").set(queue, noise)
    fn()
    return np.ascontiguousarray(fn.buffer("flags").get(queue).T)


def check(context, queue, oracle, dev, noise, n_sigma, n_windows, flag_value=1, pad=0):
    out = run_cm(context, queue, dev, noise, n_sigma, n_windows, flag_value, pad)
    expected = oracle.ThresholdSumHost(n_sigma, n_windows, flag_value=flag_value)(dev, noise)
    np.testing.assert_array_equal(expected, out)
    np.testing.assert_array_equal(run_bm(context, queue, dev, noise, n_sigma, n_windows,
                                         flag_value), out)  # fmt: skip
    return out


def interference(channels, baselines, seed):
    """Unit noise with 2 % strong spikes and, per baseline, a broad weak run that only
    the wide windows find; noise estimates near 1."""
    rs = np.random.RandomState(seed)
    dev = rs.standard_normal((channels, baselines)).astype(np.float32)
    dev[rs.random_sample((channels, baselines)) < 0.02] += 40.0
    if channels > 8:
        starts = rs.randint(0, max(1, channels - 40), baselines)
        lengths = rs.randint(3, 41, baselines)
        for b in range(min(baselines, 4096)):
            dev[starts[b] : starts[b] + lengths[b], b] += np.float32(2.5 + 3.5 * rs.random_sample())
    noise = (0.9 + 0.2 * rs.random_sample(baselines)).astype(np.float32)
    return dev, noise


@pytest.mark.parametrize("n_windows", range(1, 9))
@pytest.mark.parametrize("channels", CHANNELS)
def test_shapes(n_windows, channels, context, command_queue, oracle):
    for baselines in BASELINES:
        dev, noise = interference(channels, baselines, seed=channels * 10 + n_windows)
        flag_value = 1 if baselines % 2 else 7
        out = check(context, command_queue, oracle, dev, noise, 6.0, n_windows, flag_value,
                    pad=0 if baselines == 64 else 29)  # fmt: skip
        if channels >= 255:
            assert np.count_nonzero(out) > 0


@pytest.mark.parametrize("n_windows", range(1, 9))
def test_long_band(n_windows, context, command_queue, oracle):
    dev, noise = interference(32768, 65, seed=100 + n_windows)
    check(context, command_queue, oracle, dev, noise, 6.0, n_windows, 3, pad=3)


@pytest.mark.parametrize("n_windows", [1, 4, 5, 8])
@pytest.mark.parametrize("channels", [7, 256, 1000])
def test_many_baselines(n_windows, channels, context, command_queue, oracle):
    dev, noise = interference(channels, 70000, seed=200 + n_windows)
    check(context, command_queue, oracle, dev, noise, 6.0, n_windows, 1, pad=16)


@pytest.mark.parametrize("n_windows", range(1, 9))
def test_wide_combs(n_windows, context, command_queue, oracle):
    """Broad weak interference that only the wide windows find (inputs.py)."""
    dev, noise = inputs.threshold_wide_case()
    check(context, command_queue, oracle, dev, noise, 4.0, n_windows, 2)


@pytest.mark.parametrize("n_windows", [1, 2, 4, 6, 8])
def test_specials(n_windows, context, command_queue, oracle):
    """NaN and +-inf deviations, fully flagged stretches, a huge downward deviation, and
    thresholds that are zero, negative or NaN."""
    dev, noise = inputs.threshold_wide_case()
    dev = dev.copy()
    noise = noise.copy()
    dev[5, :] = np.nan
    dev[6, ::3] = np.inf
    dev[7, 1::3] = -np.inf
    dev[100:230, 7:11] = 500.0  # a stretch every window flags
    dev[40, 20] = -1e30
    dev[:, 30] = np.nan
    noise[12] = 0.0  # threshold 0: every positive window fires
    noise[13] = -1.0  # negative threshold
    noise[14] = np.nan  # never fires
    noise[15] = np.inf
    check(context, command_queue, oracle, dev, noise, 6.0, n_windows, 1, pad=5)
    check(context, command_queue, oracle, dev, noise, 0.0, n_windows, 1)
    check(context, command_queue, oracle, dev, noise, -2.0, n_windows, 1)


def test_threshold_host_from_device(context, command_queue, oracle):
    from katsdpsigproc_amd.rfi import device

    dev, noise = inputs.threshold_case()[0], None
    noise = oracle.NoiseEstMADHost()(dev).astype(np.float32)
    template = device.ThresholdSumDeviceTemplate(context, 4, transposed=False)
    out = device.ThresholdHostFromDevice(template, command_queue, 11.0)(dev, noise)
    np.testing.assert_array_equal(oracle.ThresholdSumHost(11.0, 4)(dev, noise), out)


# ---------------------------------------------------------------------------- flagger
def run_sequence(context, queue, vis, flags, mode, width, transposed, noise_est):
    from katsdpsigproc_amd.rfi import device

    if noise_est == "MAD":
        ne = device.NoiseEstMADDeviceTemplate(context, tuning={"method": 0})
    else:
        ne = device.NoiseEstMADTDeviceTemplate(context, vis.shape[0])
    template = device.FlaggerDeviceTemplate(
        device.BackgroundMedianFilterDeviceTemplate(context, width,
                                                    use_flags=device.BackgroundFlags[mode]),
        ne,
        device.ThresholdSumDeviceTemplate(context, 4, transposed=transposed),
        fused=False,
    )  # fmt: skip
    fn = template.instantiate(queue, *vis.shape, threshold_args=dict(n_sigma=11.0))
    assert isinstance(fn, device.FlaggerDevice)
    if not transposed:
        assert "flags_t" not in fn.slots
        assert ("deviations_t" in fn.slots) == (noise_est == "MADT")
    fn.ensure_all_bound()
    fn.buffer("vis").set(queue, vis)
    if flags is not None:
        fn.buffer("input_flags").set(queue, flags)
    fn()
    return fn.buffer("flags").get(queue), fn.buffer("noise").get(queue)


def expected_sequence(oracle, vis, flags, width):
    """The oracle's FlaggerHost stages with the sequence's float32 intermediates."""
    dev32 = oracle.BackgroundMedianFilterHost(width)(vis, flags).astype(np.float32)
    noise32 = oracle.NoiseEstMADHost()(dev32).astype(np.float32)
    return oracle.ThresholdSumHost(11.0, 4)(dev32, noise32), noise32


class TestFlagger:
    @pytest.fixture(scope="class")
    def blocks(self):
        out = {}
        for channels, baselines, seed in ((4096, 160, 21), (16384, 96, 23)):
            vis = inputs.add_rfi(inputs.generate_data(channels, baselines, seed=seed), seed=seed + 1)
            rs = np.random.RandomState(seed=seed + 2)
            flags = (rs.random_sample(vis.shape) < 1.0 / 16.0).astype(np.uint8)
            out[channels] = (vis, flags)
        return out

    @pytest.mark.parametrize("mode", ["NONE", "CHANNEL", "FULL"])
    @pytest.mark.parametrize("channels, width", [(4096, 63), (16384, 13), (16384, 63)])
    def test_sequence(self, channels, width, mode, blocks, context, command_queue, oracle):
        vis, full = blocks[channels]
        flags = {"NONE": None, "CHANNEL": np.ascontiguousarray(full[:, 0]), "FULL": full}[mode]
        expected, noise32 = expected_sequence(oracle, vis, flags, width)
        assert expected.sum() > 0
        for noise_est in ("MAD", "MADT"):
            out_flags, out_noise = run_sequence(context, command_queue, vis, flags, mode, width,
                                                False, noise_est)  # fmt: skip
            np.testing.assert_array_equal(noise32, out_noise)
            np.testing.assert_array_equal(expected, out_flags)
        ref_flags, _ = run_sequence(context, command_queue, vis, flags, mode, width, True, "MADT")
        np.testing.assert_array_equal(ref_flags, out_flags)
