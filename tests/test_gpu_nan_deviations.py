"""NaN deviations on the GPU: the stand-alone noise estimates on every path of ``ksp_madnz_t``
and ``ksp_madnz`` and the baseline-major thresholds, exact against ``rfi.host`` (by which a
NaN deviation takes no part in the median, a window holding a NaN never fires and a NaN sample
is never flagged), and NaN amplitudes through the background filter and the flaggers against
the CPU oracle. A NaN expected must come out as a NaN; its payload is free. The inputs are
those of tests/inputs_nan_deviations.py, whose claims tests/test_nan_deviations.py checks."""

import ctypes
import functools
import warnings

import numpy as np
import pytest

from katsdpsigproc_amd import _lib
from tests import inputs, inputs_nan_deviations as nd, subviews

pytestmark = pytest.mark.gpu

CHANNELS = nd.MAD_CHANNELS  # below, at and above every change of path of csrc/noise.hip
COLUMNS = nd.MAD_COLUMNS


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


@functools.lru_cache(maxsize=None)
def mad_case(channels):
    """(deviations [channels][COLUMNS], the host's noise as float32), built once per length and
    shared by the tests of that length (read-only)."""
    from katsdpsigproc_amd.rfi import host

    dev = nd.nan_mad_case(channels, COLUMNS)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # "no non-zero deviations"
        want = host.NoiseEstMADHost()(dev).astype(np.float32)
    dev.setflags(write=False)
    want.setflags(write=False)
    return dev, want


def check_noise(want, out, channels, what):
    """Exact; the message names the first differing column, its class and both values."""
    assert out.dtype == np.float32 and out.shape == want.shape
    bad = np.flatnonzero(~((want == out) | (np.isnan(want) & np.isnan(out))))
    if bad.size:
        b = int(bad[0])
        classes = sorted({nd.column_class(channels, int(c)) for c in bad})
        raise AssertionError(
            f"{what}, {channels} channels: {bad.size} of {want.size} columns differ (classes "
            f"{classes}); first column {b} ({nd.column_class(channels, b)}): host "
            f"{want[b]!r}, kernel {out[b]!r}")  # fmt: skip


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


@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("method", ["T", 0, 1])
def test_noise(method, channels, context, command_queue):
    """NoiseEstMADTDeviceTemplate ("T") and NoiseEstMADDeviceTemplate with `method` 0 and 1."""
    dev, want = mad_case(channels)
    out = run_noise(context, command_queue, dev, method)
    check_noise(want, out, channels, f"method {method}")


@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("launcher", ["ksp_madnz_t", "ksp_madnz"])
def test_noise_raw_subview(launcher, channels, context, command_queue):
    """The raw launchers on a sub-view with an odd stride and a pointer 4 bytes off a 16-byte
    boundary: the element-wise load branches. The input lies in NaN poison and must be left
    alone; the output lies in sentinels."""
    dev, want = mad_case(channels)
    data = np.ascontiguousarray(dev.T) if launcher == "ksp_madnz_t" else dev
    cols = data.shape[1]
    stride = -(-cols // 16) * 16 + 1
    src = subviews.DeviceView(context, command_queue, np.float32, data, stride, 1, poison=True)
    assert src.address % 16 == 4 and src.stride % 2 == 1
    blank = subviews.sentinel_array((1, COLUMNS), np.float32)
    noise = subviews.DeviceView(context, command_queue, np.float32, blank, COLUMNS, 1)
    _lib.call(launcher, context.device.index, ctypes.c_void_p(command_queue.stream), src.ptr,
              noise.ptr, channels, COLUMNS, src.stride)  # fmt: skip
    out = noise.read("noise")[0]
    src.read("in")
    check_noise(want, out, channels, launcher)


@pytest.mark.parametrize("channels", nd.GOLDEN_CHANNELS)
@pytest.mark.parametrize("method", ["T", 0, 1])
def test_noise_reference_golden(method, channels, context, command_queue):
    """Against the recorded output of the reference's own NoiseEstMADHost."""
    golden = np.load(nd.GOLDEN, allow_pickle=False)[f"mad_nan_{channels}"].astype(np.float32)
    dev, want = mad_case(channels)
    out = run_noise(context, command_queue, dev, method)
    check_noise(golden, out, channels, f"reference golden, method {method}")
    check_noise(want, out, channels, f"method {method}")


@pytest.mark.parametrize("kind", ["MAD", "MADT"])
def test_noise_host_from_device(kind, context, command_queue):
    """The host adapter, which callers with their own NumPy deviations use."""
    from katsdpsigproc_amd.rfi import device

    channels = 4097
    dev, want = mad_case(channels)
    template = (device.NoiseEstMADDeviceTemplate(context) if kind == "MAD"
                else device.NoiseEstMADTDeviceTemplate(context, 10240))  # fmt: skip
    out = device.NoiseEstHostFromDevice(template, command_queue)(dev)
    check_noise(want, out, channels, f"NoiseEstHostFromDevice, {kind}")


# ------------------------------------------------------------------------------ thresholds
@functools.lru_cache(maxsize=2)
def threshold_case(channels):
    dev, noise = nd.nan_threshold_case(channels)
    dev.setflags(write=False)
    noise.setflags(write=False)
    return dev, noise


def check_flags(want, out, what):
    assert out.dtype == np.uint8 and out.shape == want.shape
    bad = np.argwhere(want != out)
    assert not bad.size, (f"{what}: {len(bad)} flags differ, first at channel {bad[0][0]}, "
                          f"column {bad[0][1]}: host {want[tuple(bad[0])]}, kernel {out[tuple(bad[0])]}")  # fmt: skip


@pytest.mark.parametrize("channels", nd.THRESHOLD_CHANNELS)
@pytest.mark.parametrize("transposed", [True, False])
def test_threshold_simple(transposed, channels, context, command_queue):
    from katsdpsigproc_amd.rfi import device, host

    dev, noise = threshold_case(channels)
    template = device.ThresholdSimpleDeviceTemplate(context, transposed)
    fn = template.instantiate(command_queue, channels, dev.shape[1], nd.THRESHOLD_N_SIGMA)
    fn.ensure_all_bound()
    fn.buffer("deviations").set(command_queue, np.ascontiguousarray(dev.T) if transposed else dev)
    fn.buffer("noise").set(command_queue, noise)
    fn.buffer("flags").set(command_queue, np.full(dev.shape[::-1] if transposed else dev.shape,
                                                  255, np.uint8))  # fmt: skip
    fn()
    out = fn.buffer("flags").get(command_queue)
    out = np.ascontiguousarray(out.T) if transposed else out
    want = host.ThresholdSimpleHost(nd.THRESHOLD_N_SIGMA)(dev, noise)
    check_flags(want, out, f"simple, transposed {transposed}")
    assert want.any() and not out[np.isnan(dev)].any()


@pytest.mark.parametrize("channels", nd.THRESHOLD_CHANNELS)
@pytest.mark.parametrize("n_windows", range(1, 9))
@pytest.mark.parametrize("vt", [8, 16, 32])
def test_threshold_sum(vt, n_windows, channels, context, command_queue):
    """ksp_threshold_sum with 8, 16 and 32 channels per thread (2100 channels are two chunks
    with a halo at 8, one chunk otherwise) against rfi.host.ThresholdSumHost."""
    from katsdpsigproc_amd.rfi import device, host

    dev, noise = threshold_case(channels)
    template = device.ThresholdSumDeviceTemplate(context, n_windows, 1, {"vt": vt})
    fn = template.instantiate(command_queue, channels, dev.shape[1], nd.THRESHOLD_N_SIGMA)
    fn.ensure_all_bound()
    fn.buffer("deviations").set(command_queue, np.ascontiguousarray(dev.T))
    fn.buffer("noise").set(command_queue, noise)
    fn.buffer("flags").set(command_queue, np.full(dev.shape[::-1], 255, np.uint8))
    fn()
    out = np.ascontiguousarray(fn.buffer("flags").get(command_queue).T)
    want = host.ThresholdSumHost(nd.THRESHOLD_N_SIGMA, n_windows)(dev, noise)
    check_flags(want, out, f"sum, vt {vt}, {n_windows} windows")
    assert want.any() and not out[np.isnan(dev)].any()


# ------------------------------------------------------------------- NaN amplitudes
def run_background(context, queue, amp, fl, width):
    from katsdpsigproc_amd.rfi import device

    mode = "NONE" if fl is None else "FULL"
    template = device.BackgroundMedianFilterDeviceTemplate(context, width, True,
                                                           device.BackgroundFlags[mode])  # fmt: skip
    fn = template.instantiate(queue, *amp.shape)
    fn.ensure_all_bound()
    fn.buffer("vis").set(queue, amp)
    if fl is not None:
        fn.buffer("flags").set(queue, fl)
    fn()
    return fn.buffer("deviations").get(queue)


@pytest.mark.parametrize("mode", ["none", "full"])
@pytest.mark.parametrize("width", [5, 13, 63])
def test_amplitude_background(width, mode, context, command_queue, oracle):
    amp, in_flags = inputs.nonfinite_amp_nan_case()
    fl = None if mode == "none" else in_flags
    out = run_background(context, command_queue, amp, fl, width)
    expected = oracle.BackgroundMedianFilterHost(width, True)(amp, fl)
    with np.errstate(over="ignore"):
        np.testing.assert_array_equal(expected.astype(np.float32), out)
    assert not np.isnan(out).any() and (out[np.isnan(amp)] == 0).all()


def run_flagger(context, queue, amp, fl, fused, noise="MADT"):
    from katsdpsigproc_amd.rfi import device

    mode = "NONE" if fl is None else "FULL"
    bg = device.BackgroundMedianFilterDeviceTemplate(context, 13, True, device.BackgroundFlags[mode])
    ne = (device.NoiseEstMADTDeviceTemplate(context, max(amp.shape[0], 1024)) if noise == "MADT"
          else device.NoiseEstMADDeviceTemplate(context))  # fmt: skip
    th = device.ThresholdSumDeviceTemplate(context, 4)
    template = device.FlaggerDeviceTemplate(bg, ne, th, fused=fused, keep_deviations=True)
    fn = template.instantiate(queue, *amp.shape, threshold_args={"n_sigma": 11.0})
    assert isinstance(fn, device.FusedFlaggerDevice) == fused
    fn.ensure_all_bound()
    fn.buffer("vis").set(queue, amp)
    if fl is not None:
        fn.buffer("input_flags").set(queue, fl)
    fn.buffer("flags").set(queue, np.full(amp.shape, 255, np.uint8))
    fn()
    path = _lib.call("ksp_flagger_fused_last_path") if fused else None
    return (fn.buffer("flags").get(queue), fn.buffer("noise").get(queue),
            fn.buffer("deviations").get(queue), path)  # fmt: skip


def check_flagger(oracle, amp, fl, flags, noise, dev):
    with np.errstate(all="ignore"):
        want_flags, want_noise, want_dev = oracle.flagger_full(
            amp, fl, width=13, amplitudes=True, n_windows=4, n_sigma=11.0, want_deviations=True)
    np.testing.assert_array_equal(want_dev.astype(np.float32), dev)
    np.testing.assert_array_equal(want_noise.astype(np.float32), noise)
    np.testing.assert_array_equal(want_flags, flags)
    assert not flags[np.isnan(amp)].any()


@pytest.mark.parametrize("mode", ["none", "full"])
@pytest.mark.parametrize("channels, path", [(1024, _lib.FUSED_PATH_STRIP), (8192, _lib.FUSED_PATH_LONG)])
def test_amplitude_fused(channels, path, mode, context, command_queue, oracle):
    """The fused flagger: the strip kernel at 1024 channels and the long kernel at 8192."""
    amp, in_flags = inputs.nonfinite_amp_nan_case(channels)
    fl = None if mode == "none" else in_flags
    flags, noise, dev, took = run_flagger(context, command_queue, amp, fl, True)
    assert took == path, took
    check_flagger(oracle, amp, fl, flags, noise, dev)


@pytest.mark.parametrize("noise", ["MAD", "MADT"])
@pytest.mark.parametrize("channels", [1024, 8192])
def test_amplitude_sequence(channels, noise, context, command_queue, oracle):
    """The kernel-per-stage sequence (background, noise estimate, SumThreshold)."""
    amp, in_flags = inputs.nonfinite_amp_nan_case(channels)
    flags, noise_out, dev, _ = run_flagger(context, command_queue, amp, in_flags, False, noise)
    check_flagger(oracle, amp, in_flags, flags, noise_out, dev)
