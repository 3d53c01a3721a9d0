"""Infinite (and NaN) input on every kernel that computes a median or consumes deviations,
bit for bit against the CPU oracle and, at the shapes of the fixture, against the golden
vectors of the reference (tests/golden/make_golden_nonfinite.py).

The reference's rolling median leaves +-inf amplitudes out of every window (pandas turns
them into NaN first), while their own deviation is inf - median, and 0 when no finite
sample is left in the window."""

import numpy as np
import pytest

from katsdpsigproc_amd import _lib
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


@pytest.fixture(scope="module")
def golden():
    return inputs.nonfinite_golden()


def unpack(bits, shape):
    n = int(np.prod(shape))
    return np.unpackbits(bits)[:n].reshape(shape).astype(np.uint8)


def mode_flags(in_flags, mode, chan_col):
    return {"none": None, "channel": in_flags[:, chan_col], "full": in_flags}[mode]


def run_flagger(context, queue, vis, fl, *, width=13, amplitudes=False, noise="MADT",
                n_windows=4, keep_deviations=True, fused=True, n_sigma=11.0):  # fmt: skip
    """The flagger on `vis`; returns (outputs, ksp_flagger_fused_last_path)."""
    from katsdpsigproc_amd.rfi import device

    mode = "NONE" if fl is None else ("CHANNEL" if fl.ndim == 1 else "FULL")
    bg = device.BackgroundMedianFilterDeviceTemplate(context, width, amplitudes,
                                                     device.BackgroundFlags[mode])  # fmt: skip
    ne = (device.NoiseEstMADTDeviceTemplate(context, max(vis.shape[0], 1024)) if noise == "MADT"
          else device.NoiseEstMADDeviceTemplate(context))  # fmt: skip
    th = device.ThresholdSumDeviceTemplate(context, n_windows)
    template = device.FlaggerDeviceTemplate(bg, ne, th, fused=fused, keep_deviations=keep_deviations)
    fn = template.instantiate(queue, *vis.shape, threshold_args={"n_sigma": n_sigma})
    assert isinstance(fn, device.FusedFlaggerDevice) == fused
    fn.ensure_all_bound()
    fn.buffer("vis").set(queue, vis)
    if fl is not None:
        fn.buffer("input_flags").set(queue, fl)
    fn.buffer("flags").set(queue, np.full(vis.shape, 255, np.uint8))
    fn()
    path = _lib.call("ksp_flagger_fused_last_path") if fused else None
    out = {"flags": fn.buffer("flags").get(queue), "noise": fn.buffer("noise").get(queue)}
    if keep_deviations:
        out["deviations"] = fn.buffer("deviations").get(queue)
    return out, path


def check_oracle(oracle, out, vis, fl, *, width=13, amplitudes=False, n_windows=4, n_sigma=11.0):
    with np.errstate(all="ignore"):
        flags, noise, dev = oracle.flagger_full(vis, fl, width=width, amplitudes=amplitudes,
                                                n_windows=n_windows, n_sigma=n_sigma,
                                                want_deviations=True)  # fmt: skip
    if "deviations" in out:
        np.testing.assert_array_equal(dev.astype(np.float32), out["deviations"])
    np.testing.assert_array_equal(noise.astype(np.float32), out["noise"])
    np.testing.assert_array_equal(flags, out["flags"])


def check_golden(golden, out, key, rows, shape):
    np.testing.assert_array_equal(golden[key + "_noise"].astype(np.float32), out["noise"])
    np.testing.assert_array_equal(unpack(golden[key + "_flags"], shape), out["flags"])
    if "deviations" in out and key.endswith("_none"):
        np.testing.assert_array_equal(golden[key + "_dev_rows"].astype(np.float32),
                                      out["deviations"][rows])  # fmt: skip


class TestFused:
    @pytest.mark.parametrize("n_windows", [4, 8])
    @pytest.mark.parametrize("mode", ["none", "channel", "full"])
    @pytest.mark.parametrize("width", [5, 13, 31])
    def test_strip_kernel(self, width, mode, n_windows, context, command_queue, oracle, golden):
        """4096 channels, the 4-baseline kernel (path 1): every strip holds an infinity
        except the clean control's, and takes the sorted window."""
        vis, in_flags, _, rows, chan_col = inputs.nonfinite_input("cplx")
        fl = mode_flags(in_flags, mode, chan_col)
        out, path = run_flagger(context, command_queue, vis, fl, width=width, n_windows=n_windows)
        assert path == _lib.FUSED_PATH_STRIP, path
        check_oracle(oracle, out, vis, fl, width=width, n_windows=n_windows)
        if n_windows == 4:
            check_golden(golden, out, f"cplx_w{width}_{mode}", rows, vis.shape)

    def test_ring_kernel(self, context, command_queue, oracle, golden):
        vis, _, _, rows, _ = inputs.nonfinite_input("cplx")
        with _lib.fused_ring_mode(1):
            out, path = run_flagger(context, command_queue, vis, None, keep_deviations=False)
        assert path & _lib.FUSED_PATH_RING, path
        check_oracle(oracle, out, vis, None)
        check_golden(golden, out, "cplx_w13_none", rows, vis.shape)

    @pytest.mark.parametrize("amplitudes", [False, True])
    @pytest.mark.parametrize("channels", [8192, 12288])
    def test_long_kernel(self, channels, amplitudes, context, command_queue, oracle):
        """More than 4096 channels (path 2), infinities on the group boundaries; amplitude
        input with +-inf and negative amplitudes in one strip."""
        if amplitudes:
            vis, _ = inputs.nonfinite_amp_case(channels)
            vis[4095:4098, 4] = [np.inf, -np.inf, np.inf]
        else:
            vis, _ = inputs.nonfinite_case(channels)
            vis[[4095, 4096, 8191, 8192 % channels], 5] = np.inf
        out, path = run_flagger(context, command_queue, vis, None, amplitudes=amplitudes)
        assert path == _lib.FUSED_PATH_LONG, path
        check_oracle(oracle, out, vis, None, amplitudes=amplitudes)

    def test_amplitude_input_golden(self, context, command_queue, oracle, golden):
        vis, in_flags, _, rows, _ = inputs.nonfinite_input("amp")
        for mode, fl in (("none", None), ("full", in_flags)):
            out, path = run_flagger(context, command_queue, vis, fl, amplitudes=True)
            assert path == _lib.FUSED_PATH_STRIP, path
            check_oracle(oracle, out, vis, fl, amplitudes=True)
            check_golden(golden, out, f"amp_w13_{mode}", rows, vis.shape)


def run_background(context, queue, vis, fl, width, amplitudes, csplit=0):
    from katsdpsigproc_amd.rfi import device

    mode = "NONE" if fl is None else ("CHANNEL" if fl.ndim == 1 else "FULL")
    template = device.BackgroundMedianFilterDeviceTemplate(
        context, width, amplitudes, device.BackgroundFlags[mode],
        tuning={"wgs": 64, "csplit": csplit},
    )  # fmt: skip
    fn = template.instantiate(queue, *vis.shape)
    fn.ensure_all_bound()
    fn.buffer("vis").set(queue, vis)
    if fl is not None:
        fn.buffer("flags").set(queue, fl)
    fn()
    return fn.buffer("deviations").get(queue)


class TestBackground:
    # csplit 41: segments of 100 channels, which start on the planted samples at 500, 800,
    # 1000, 1200, 1500, 1600, 2000, 2500, 3000, 3500 and 3800; csplit 64: segments of 64
    # channels, starting at the lane-boundary infinities 64 and 128
    @pytest.mark.parametrize("csplit", [0, 41, 64])
    @pytest.mark.parametrize("mode", ["none", "full"])
    @pytest.mark.parametrize("tag", ["cplx", "amp"])
    @pytest.mark.parametrize("width", [5, 13, 63, 255])
    def test_background(self, width, tag, mode, csplit, context, command_queue, oracle, golden):
        vis, in_flags, amplitudes, rows, chan_col = inputs.nonfinite_input(tag)
        fl = mode_flags(in_flags, mode, chan_col)
        out = run_background(context, command_queue, vis, fl, width, amplitudes, csplit)
        expected = oracle.BackgroundMedianFilterHost(width, amplitudes)(vis, fl)
        with np.errstate(over="ignore"):
            np.testing.assert_array_equal(expected.astype(np.float32), out)
        if mode == "none":
            np.testing.assert_array_equal(
                golden[f"{tag}_w{width}_none_dev_rows"].astype(np.float32), out[rows])


def run_noise(context, queue, dev, method):
    from katsdpsigproc_amd.rfi import device

    channels, baselines = dev.shape
    if method == "T":
        fn = device.NoiseEstMADTDeviceTemplate(context, channels).instantiate(queue, channels, baselines)
        data = np.ascontiguousarray(dev.T)
    else:
        template = device.NoiseEstMADDeviceTemplate(context, tuning={"method": method})
        fn = template.instantiate(queue, channels, baselines)
        data = dev
    fn.ensure_all_bound()
    fn.buffer("deviations").set(queue, data)
    fn()
    return fn.buffer("noise").get(queue)


@pytest.mark.parametrize("channels", inputs.NONFINITE_MAD_CHANNELS)
@pytest.mark.parametrize("method", [0, 1, "T"])
def test_mad(method, channels, context, command_queue, oracle, golden):
    """+-inf deviations, more than half and exactly half of them inf, median |d| above
    FLT_MAX / 2 with odd and even counts; short bands and the long-band kernels."""
    dev = inputs.nonfinite_mad_case(channels)
    out = run_noise(context, command_queue, dev, method)
    np.testing.assert_array_equal(oracle.NoiseEstMADHost()(dev).astype(np.float32), out)
    np.testing.assert_array_equal(golden[f"mad_{channels}"].astype(np.float32), out)


def run_threshold(context, queue, dev, noise, kind, transposed, n_windows=4):
    from katsdpsigproc_amd.rfi import device

    channels, baselines = dev.shape
    if kind == "sum":
        template = device.ThresholdSumDeviceTemplate(context, n_windows, transposed=transposed)
    else:
        template = device.ThresholdSimpleDeviceTemplate(context, transposed)
    fn = template.instantiate(queue, channels, baselines, 11.0)
    fn.ensure_all_bound()
    fn.buffer("deviations").set(queue, np.ascontiguousarray(dev.T) if transposed else dev)
    fn.buffer("noise").set(queue, noise)
    fn()
    flags = fn.buffer("flags").get(queue)
    return np.ascontiguousarray(flags.T) if transposed else flags


@pytest.mark.parametrize("transposed", [True, False])
@pytest.mark.parametrize("n_windows", range(1, 9))
def test_threshold_sum(n_windows, transposed, context, command_queue, oracle, golden):
    dev, noise = inputs.nonfinite_threshold_case()
    out = run_threshold(context, command_queue, dev, noise, "sum", transposed, n_windows)
    np.testing.assert_array_equal(oracle.ThresholdSumHost(11.0, n_windows=n_windows)(dev, noise), out)
    np.testing.assert_array_equal(unpack(golden[f"threshold_sum_w{n_windows}"], dev.shape), out)


@pytest.mark.parametrize("transposed", [True, False])
def test_threshold_simple(transposed, context, command_queue, oracle, golden):
    dev, noise = inputs.nonfinite_threshold_case()
    out = run_threshold(context, command_queue, dev, noise, "simple", transposed)
    np.testing.assert_array_equal(oracle.ThresholdSimpleHost(11.0)(dev, noise), out)
    np.testing.assert_array_equal(unpack(golden["threshold_simple"], dev.shape), out)


@pytest.mark.parametrize("channels", [4096, 32768])
@pytest.mark.parametrize("noise", ["MAD", "MADT"])
def test_sequence(noise, channels, context, command_queue, oracle, golden):
    """The kernel-per-stage flagger (background, noise estimate, SumThreshold)."""
    vis, in_flags = inputs.nonfinite_case(channels)
    out, _ = run_flagger(context, command_queue, vis, in_flags, noise=noise, fused=False,
                         keep_deviations=False)  # fmt: skip
    check_oracle(oracle, out, vis, in_flags)
    if channels == inputs.NONFINITE_CHANNELS:
        check_golden(golden, out, "cplx_w13_full", None, vis.shape)
