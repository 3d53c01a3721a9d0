"""Wide median windows (odd widths 33 to 255) on the GPU: the background operation and the
kernel-per-stage flagger built on it, bit for bit against the CPU oracle."""

import numpy as np
import pytest

from tests import inputs

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


def run_background(context, queue, vis, flags=None, width=63, amplitudes=False, mode=None,
                   csplit=0, pad=0):  # fmt: skip
    """The standalone operation on `vis` (rows padded by `pad` elements if asked)."""
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import device

    if mode is None:
        mode = "NONE" if flags is None else ("CHANNEL" if flags.ndim == 1 else "FULL")
    template = device.BackgroundMedianFilterDeviceTemplate(
        context, width, amplitudes, device.BackgroundFlags[mode],
        tuning={"wgs": 64, "csplit": csplit},
    )  # fmt: skip
    fn = template.instantiate(queue, *vis.shape)
    if pad:
        dim = fn.slots["vis"].dimensions[1]
        accel.Dimension(dim.size, min_padded_size=dim.size + pad).link(dim)
    fn.ensure_all_bound()
    assert fn.buffer("vis").padded_shape[1] >= vis.shape[1] + pad
    fn.buffer("vis").set(queue, vis)
    if flags is not None:
        fn.buffer("flags").set(queue, flags)
    fn()
    return fn.buffer("deviations").get(queue)


def check(oracle, out, vis, flags=None, width=63, amplitudes=False):
    expected = oracle.BackgroundMedianFilterHost(width, amplitudes)(vis, flags)
    with np.errstate(invalid="ignore", over="ignore"):
        np.testing.assert_array_equal(expected.astype(np.float32), out)


# the smallest and the largest width of every kernel instantiation (5, 8, 16, 24 and 32 slots
# per lane: up to 39, 63, 127, 191, 255), and 35
WIDTHS = [33, 35, 39, 41, 63, 65, 127, 129, 191, 193, 255]


class TestWideBackground:
    @pytest.mark.parametrize("amplitudes", [False, True])
    @pytest.mark.parametrize("mode", ["NONE", "CHANNEL", "FULL"])
    @pytest.mark.parametrize("width", WIDTHS)
    def test_background_case(self, width, mode, amplitudes, context, command_queue, oracle):
        vis_big, flags_big = inputs.background_case()
        vis = oracle.abs_c64(vis_big) if amplitudes else vis_big
        flags = {"NONE": None, "CHANNEL": flags_big[:, 0], "FULL": flags_big}[mode]
        out = run_background(context, command_queue, vis, flags, width, amplitudes, mode)
        check(oracle, out, vis, flags, width, amplitudes)

    @pytest.mark.parametrize(
        "channels, baselines, width, pad",
        [
            (100, 77, 255, 0),   # band narrower than the window
            (1, 5, 33, 0),       # a single channel
            (2, 3, 255, 0),
            (40, 1, 63, 0),      # one baseline: a single lane group, most of the wave idle
            (300, 131, 65, 3),   # baselines not a multiple of 8 or of 32, padded rows
            (517, 200, 129, 16),
            (1000, 9, 191, 0),
        ],
    )  # fmt: skip
    @pytest.mark.parametrize("mode", ["NONE", "FULL"])
    def test_ragged_shapes(self, channels, baselines, width, pad, mode, context, command_queue,
                           oracle):  # fmt: skip
        vis = inputs.generate_data(channels, baselines, seed=channels + baselines)
        flags = None
        if mode == "FULL":
            rs = np.random.RandomState(channels)
            flags = (rs.random_sample(vis.shape) < 0.1).astype(np.uint8)
        out = run_background(context, command_queue, vis, flags, width, pad=pad)
        check(oracle, out, vis, flags, width)

    @pytest.mark.parametrize("width", [33, 127, 255])
    def test_channel_splits_agree(self, width, context, command_queue, oracle):
        """The split only changes who computes what, down to a single segment and to a
        band narrower than the window."""
        vis_big, flags_big = inputs.background_case()
        outs = [
            run_background(context, command_queue, vis_big, flags_big, width, csplit=csplit)
            for csplit in (1, 8, 64)
        ]
        for out in outs[1:]:
            np.testing.assert_array_equal(outs[0], out)
        check(oracle, outs[0], vis_big, flags_big, width)
        narrow = vis_big[: width // 2]
        outs = [
            run_background(context, command_queue, narrow, None, width, csplit=csplit)
            for csplit in (1, 8, 64)
        ]
        for out in outs[1:]:
            np.testing.assert_array_equal(outs[0], out)
        check(oracle, outs[0], narrow, None, width)

    @pytest.mark.parametrize("width", [33, 64 + 1, 255])
    def test_degenerate_data(self, width, context, command_queue, oracle):
        """All-flagged baselines, even valid counts, heavy ties, zeros, subnormals, NaN, +inf
        and visibilities whose |z| overflows."""
        channels, baselines = 600, 48
        rs = np.random.RandomState(width)
        amp = rs.standard_normal((channels, baselines)).astype(np.float32)
        amp[:, 8:16] = np.round(amp[:, 8:16] * 2) / 2  # quantised: heavy ties
        amp[:, 16:20] = 0.0
        amp[::3, 20:24] = 0.0
        amp[:, 24:28] = (rs.randint(0, 6, (channels, 4)) * 2.0**-149).astype(np.float32)
        nan_mask = rs.random_sample((channels, baselines)) < 0.05
        amp[:, 28:32][nan_mask[:, 28:32]] = np.nan
        amp[100:140, 32:36] = np.inf
        amp[::7, 36:40] = np.inf
        vis = (amp * np.exp(2j * np.pi * rs.random_sample(amp.shape))).astype(np.complex64)
        vis[np.isinf(amp)] = np.inf
        vis[:, 40:44] = np.complex64(complex(3e38, 3e38))  # |z| overflows to inf
        vis[::2, 44:48] = np.complex64(complex(2e38, -3e38))
        flags = (rs.random_sample((channels, baselines)) < 0.5).astype(np.uint8)  # even counts
        flags[:, 0:4] = 1  # all flagged
        flags[:, 8:48] = 0
        flags[::5, 44:48] = 7
        out = run_background(context, command_queue, vis, flags, width)
        check(oracle, out, vis, flags, width)
        assert np.all(out[:, 0:4] == 0)
        out = run_background(context, command_queue, vis, None, width)
        check(oracle, out, vis, None, width)
        a = oracle.abs_c64(vis)
        out = run_background(context, command_queue, a, flags, width, amplitudes=True)
        check(oracle, out, a, flags, width, amplitudes=True)

    def test_full_band(self, context, command_queue, oracle):
        """4096 x 8192 at width 33 (the reference's autotuning shape), every deviation."""
        vis = inputs.add_rfi_sparse(inputs.generate_data(4096, 8192, seed=31), seed=32)
        out = run_background(context, command_queue, vis, None, 33)
        check(oracle, out, vis, None, 33)

    @pytest.mark.parametrize("width", [127, 255])
    def test_large_oracle_bounded(self, width, context, command_queue, oracle):
        """About a million samples, channel flags, the launcher's own split."""
        vis = inputs.add_rfi(inputs.generate_data(2048, 512, seed=width), seed=width + 1)
        flags = inputs.channel_mask(2048)
        out = run_background(context, command_queue, vis, flags, width)
        check(oracle, out, vis, flags, width)

    def test_width_range(self, context):
        from katsdpsigproc_amd.rfi import device

        for width in (257, 64, 100):
            with pytest.raises(ValueError, match="3..255"):
                device.BackgroundMedianFilterDeviceTemplate(context, width)


class TestWideFlagger:
    @pytest.mark.parametrize("width", [63, 255])
    def test_sequence_matches_staged_oracle(self, width, context, command_queue, oracle):
        """Stage by stage, as test_gpu_flagger's sequence test: deviations, noise, flags."""
        from katsdpsigproc_amd.rfi import device

        vis = inputs.add_rfi(inputs.generate_data(1024, 200, seed=7), seed=8)
        bg = device.BackgroundMedianFilterDeviceTemplate(context, width)
        template = device.FlaggerDeviceTemplate(
            bg, device.NoiseEstMADTDeviceTemplate(context, 10240),
            device.ThresholdSumDeviceTemplate(context),
        )  # fmt: skip
        fn = template.instantiate(command_queue, *vis.shape, threshold_args=dict(n_sigma=11.0))
        assert isinstance(fn, device.FlaggerDevice)
        fn.ensure_all_bound()
        fn.buffer("vis").set(command_queue, vis)
        fn()
        dev32 = oracle.BackgroundMedianFilterHost(width)(vis).astype(np.float32)
        noise32 = oracle.NoiseEstMADHost()(dev32).astype(np.float32)
        flags = oracle.ThresholdSumHost(11.0)(dev32, noise32)
        np.testing.assert_array_equal(dev32, fn.buffer("deviations").get(command_queue))
        np.testing.assert_array_equal(noise32, fn.buffer("noise").get(command_queue))
        np.testing.assert_array_equal(flags, fn.buffer("flags").get(command_queue))
        assert flags.sum() > 0
        with pytest.raises(ValueError):
            device.FlaggerDeviceTemplate(
                bg, device.NoiseEstMADTDeviceTemplate(context, 10240),
                device.ThresholdSumDeviceTemplate(context), fused=True,
            ).instantiate(command_queue, *vis.shape)  # fmt: skip

    @pytest.mark.parametrize("use_flags", ["NONE", "CHANNEL", "FULL"])
    @pytest.mark.parametrize("width", [63, 255])
    def test_flagger_recovers_spikes(self, width, use_flags, context, command_queue):
        # as reference test/rfi/test_flagger.py:74-132, on a wide window
        from katsdpsigproc_amd.rfi import device

        vis, spikes, input_flags = inputs.flagger_case()
        template = device.FlaggerDeviceTemplate(
            device.BackgroundMedianFilterDeviceTemplate(
                context, width, use_flags=device.BackgroundFlags[use_flags]),
            device.NoiseEstMADDeviceTemplate(context),
            device.ThresholdSimpleDeviceTemplate(context, False),
        )  # fmt: skip
        flagger = device.FlaggerHostFromDevice(
            template, command_queue, threshold_args=dict(n_sigma=11.0)
        )
        if use_flags == "CHANNEL":
            flags = flagger(vis, input_flags[:, 0])
            bcast = np.broadcast_to(input_flags[:, 0:1], vis.shape)
            np.testing.assert_array_equal(np.where(bcast, 0, spikes), flags)
        elif use_flags == "FULL":
            flags = flagger(vis, input_flags)
            np.testing.assert_array_equal(np.where(input_flags, 0, spikes), flags)
        else:
            np.testing.assert_array_equal(spikes, flagger(vis))
