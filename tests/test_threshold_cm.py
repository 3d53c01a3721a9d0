"""SumThreshold on channel-major deviations (``ThresholdSumDeviceTemplate(transposed=False)``)
without a GPU: template and slot wiring, the exported and declared launcher, its argument
checks, and a flagger sequence that needs no transposes."""

import ctypes
import os

import numpy as np
import pytest

from tests.fakes import FakeContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from katsdpsigproc_amd import _lib, build_native

    if not os.path.exists(_lib.LIB_PATH):
        build_native.build()
    return _lib.load()


def test_default_stays_baseline_major():
    from katsdpsigproc_amd.rfi import device

    ctx = FakeContext()
    assert device.ThresholdSumDeviceTemplate.transposed is True
    assert device.ThresholdSumDevice.transposed is True
    template = device.ThresholdSumDeviceTemplate(ctx, 4, 1, {"vt": 8})
    assert template.transposed is True
    fn = template.instantiate(ctx.create_command_queue(), 100, 7, 11.0)
    assert fn.transposed is True
    assert fn.slots["deviations"].shape == (7, 100)


@pytest.mark.parametrize("n_windows", [1, 4, 8])
def test_channel_major_template_and_slots(n_windows):
    from katsdpsigproc_amd.rfi import device

    ctx = FakeContext()
    queue = ctx.create_command_queue()
    template = device.ThresholdSumDeviceTemplate(ctx, n_windows, 5, transposed=False)
    assert template.transposed is False
    assert device.ThresholdSumDeviceTemplate.transposed is True  # class attribute unchanged
    fn = template.instantiate(queue, 300, 70, 6.0)
    assert fn.transposed is False and fn.parameters()["transposed"] is False
    for name in ("deviations", "flags"):
        assert fn.slots[name].shape == (300, 70)
    assert fn.slots["noise"].shape == (70,)
    # one baseline Dimension shared by both 2-D slots and the noise, as in ThresholdSimple
    assert fn.slots["deviations"].dimensions[1] is fn.slots["flags"].dimensions[1]
    assert fn.slots["noise"].dimensions[0] is fn.slots["deviations"].dimensions[1]
    fn.ensure_all_bound()
    dev = fn.buffer("deviations")
    assert dev.padded_shape[1] >= 70
    assert fn.buffer("flags").padded_shape == dev.padded_shape
    fn()
    name, args = queue.launches[-1]
    assert name == "ksp_threshold_sum_cm"
    channels, baselines, stride = (int(a) for a in args[3:6])
    assert (channels, baselines, stride) == (300, 70, dev.padded_shape[1])
    assert float(args[6]) == 6.0
    scales = args[7]
    assert [scales[i] for i in range(n_windows)] == [
        float(np.float32(1.2**-i)) for i in range(n_windows)
    ]
    assert int(args[8]) == n_windows and int(args[9]) == 5
    assert len(args) == 10


def test_channel_major_padded_rows_reach_the_launcher():
    from katsdpsigproc_amd import accel
    from katsdpsigproc_amd.rfi import device

    ctx = FakeContext()
    queue = ctx.create_command_queue()
    fn = device.ThresholdSumDeviceTemplate(ctx, transposed=False).instantiate(queue, 17, 65, 11.0)
    dim = fn.slots["deviations"].dimensions[1]
    accel.Dimension(dim.size, min_padded_size=dim.size + 40).link(dim)
    fn.ensure_all_bound()
    fn()
    _, args = queue.launches[-1]
    assert int(args[5]) >= 105 and int(args[5]) == fn.buffer("flags").padded_shape[1]


def test_channel_major_does_not_autotune(monkeypatch):
    from katsdpsigproc_amd.rfi import device

    def refuse(*args, **kwargs):
        raise AssertionError("the channel-major launcher has nothing to tune")

    monkeypatch.setattr(device.ThresholdSumDeviceTemplate, "autotune", refuse)
    template = device.ThresholdSumDeviceTemplate(FakeContext(), 4, transposed=False)
    assert dict(template.tuning) == {}


def test_library_exports_and_header_declares(lib):
    assert hasattr(lib, "ksp_threshold_sum_cm")
    text = open(os.path.join(ROOT, "include", "katsdpsigproc_hip.h")).read()
    assert "int ksp_threshold_sum_cm(" in text
    assert lib.ksp_abi_version() == 5


def _call(lib, dev, noise, flags, channels=16, baselines=8, stride=8, scales=True,
          n_windows=4):  # fmt: skip
    sc = (ctypes.c_float * 8)(*([1.0] * 8)) if scales else None
    return lib.ksp_threshold_sum_cm(0, None, dev, noise, flags, channels, baselines, stride,
                                    6.0, sc, n_windows, 1)  # fmt: skip


def test_launcher_rejects_bad_arguments_before_device_calls(lib):
    from katsdpsigproc_amd import _lib

    buf = (ctypes.c_float * 256)()
    fl = (ctypes.c_uint8 * 256)()
    for args in ((None, buf, fl), (buf, None, fl), (buf, buf, None)):
        assert _call(lib, *args) != 0
        assert "NULL" in _lib.last_error()
    assert _call(lib, buf, buf, fl, scales=False) != 0
    assert "scales" in _lib.last_error()
    for n in (0, 9):
        assert _call(lib, buf, buf, fl, n_windows=n) != 0
        assert "n_windows" in _lib.last_error() and "1..8" in _lib.last_error()
    assert _call(lib, buf, buf, fl, baselines=8, stride=7) != 0
    assert "stride" in _lib.last_error()
    assert _call(lib, buf, buf, fl, channels=-1) != 0
    assert "shape" in _lib.last_error()


def _sequence(ctx, noise_est, transposed):
    from katsdpsigproc_amd.rfi import device

    return device.FlaggerDeviceTemplate(
        device.BackgroundMedianFilterDeviceTemplate(ctx, 63),
        noise_est,
        device.ThresholdSumDeviceTemplate(ctx, transposed=transposed),
    )


@pytest.mark.parametrize("noise_transposed", [False, True])
def test_flagger_sequence_without_transposes(noise_transposed):
    from katsdpsigproc_amd import transpose
    from katsdpsigproc_amd.rfi import device

    ctx = FakeContext()
    queue = ctx.create_command_queue()
    if noise_transposed:
        ne = device.NoiseEstMADTDeviceTemplate(ctx, 4096)
    else:
        ne = device.NoiseEstMADDeviceTemplate(ctx, tuning={"method": 0})
    template = _sequence(ctx, ne, transposed=False)
    assert template.transpose_flags is None
    assert (template.transpose_deviations is None) is not noise_transposed
    fn = template.instantiate(queue, 4096, 70, threshold_args={"n_sigma": 11.0})
    assert isinstance(fn, device.FlaggerDevice)  # width 63 is never fused
    assert "flags_t" not in fn.slots
    assert not hasattr(fn, "transpose_flags")
    names = list(fn.operations)
    assert "transpose_flags" not in names
    if not noise_transposed:
        assert "deviations_t" not in fn.slots
        assert "transpose_deviations" not in names
        assert not any(isinstance(op, transpose.Transpose) for op in fn.operations.values())
    fn.ensure_all_bound()
    fn()
    launched = [name for name, _ in queue.launches]
    assert "ksp_threshold_sum_cm" in launched and "ksp_threshold_sum" not in launched
    if not noise_transposed:
        assert "ksp_transpose" not in launched
    else:
        assert launched.count("ksp_transpose") == 1  # deviations for the noise only
    # the threshold reads the background's deviations and writes the flagger's flags
    assert fn.slots["flags"].shape == (4096, 70)


def test_baseline_major_sequence_unchanged():
    from katsdpsigproc_amd.rfi import device

    ctx = FakeContext()
    queue = ctx.create_command_queue()
    ne = device.NoiseEstMADDeviceTemplate(ctx, tuning={"method": 0})
    fn = _sequence(ctx, ne, transposed=True).instantiate(
        queue, 4096, 70, threshold_args={"n_sigma": 11.0})  # fmt: skip
    assert "flags_t" in fn.slots and "deviations_t" in fn.slots
    fn.ensure_all_bound()
    fn()
    launched = [name for name, _ in queue.launches]
    assert launched.count("ksp_transpose") == 2 and "ksp_threshold_sum" in launched


@pytest.mark.parametrize("channels", [4096, 8192])
def test_fused_choice_does_not_depend_on_layout(channels):
    from katsdpsigproc_amd.rfi import device

    ctx = FakeContext()
    for width in (13, 63):
        choices = set()
        for transposed in (True, False):
            template = device.FlaggerDeviceTemplate(
                device.BackgroundMedianFilterDeviceTemplate(ctx, width),
                device.NoiseEstMADTDeviceTemplate(ctx, channels),
                device.ThresholdSumDeviceTemplate(ctx, transposed=transposed),
            )
            choices.add(template.fusable(channels))
        assert len(choices) == 1
