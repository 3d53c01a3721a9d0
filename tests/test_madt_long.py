"""NoiseEstMADT on bands of 16385 to 262144 channels without a GPU: template wiring, the
flagger's choice of the kernel-per-stage sequence, the launcher's range check, and the
reference's golden vectors against the oracle and the host classes."""

import ctypes
import os

import numpy as np
import pytest

from tests import inputs_long
from tests.fakes import FakeContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def long_golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "rfi_host_long_golden.npz"),
                   allow_pickle=False)  # fmt: skip


@pytest.mark.parametrize("channels", [16385, 32768, 262144])
def test_long_madt_template_wires_up(channels):
    from katsdpsigproc_amd.rfi import device

    ctx = FakeContext()
    queue = ctx.create_command_queue()
    template = device.NoiseEstMADTDeviceTemplate(ctx, channels)
    fn = template.instantiate(queue, channels, 3)
    fn.ensure_all_bound()
    fn()
    name, args = queue.launches[-1]
    assert name == "ksp_madnz_t"
    assert int(args[2]) == channels and int(args[3]) == 3 and int(args[4]) >= channels


def test_long_madt_template_rejects_beyond_range():
    from katsdpsigproc_amd.rfi import device

    with pytest.raises(ValueError, match="262144"):
        device.NoiseEstMADTDeviceTemplate(FakeContext(), 262145)


def test_long_flagger_is_the_sequence():
    from katsdpsigproc_amd.rfi import device

    ctx = FakeContext()
    queue = ctx.create_command_queue()

    def template(fused=None):
        return device.FlaggerDeviceTemplate(
            device.BackgroundMedianFilterDeviceTemplate(ctx, 13),
            device.NoiseEstMADTDeviceTemplate(ctx, 32768),
            device.ThresholdSumDeviceTemplate(ctx),
            fused=fused,
        )

    assert not template().fusable(32768)
    fn = template().instantiate(queue, 32768, 16, threshold_args={"n_sigma": 11.0})
    assert isinstance(fn, device.FlaggerDevice)
    fn.ensure_all_bound()
    fn()
    madt = [args for name, args in queue.launches if name == "ksp_madnz_t"]
    assert len(madt) == 1 and int(madt[0][2]) == 32768 and int(madt[0][3]) == 16
    with pytest.raises(ValueError):
        template(fused=True).instantiate(queue, 32768, 16)


def test_channel_major_transposing_cutoff_unchanged():
    """Tuning ``method`` 1 of the channel-major estimator still stops at 16384 channels."""
    from katsdpsigproc_amd.rfi import device

    ctx = FakeContext()
    queue = ctx.create_command_queue()
    template = device.NoiseEstMADDeviceTemplate(ctx, tuning={"method": 1})
    assert "deviations_t" in template.instantiate(queue, 16384, 4).slots
    fn = template.instantiate(queue, 20000, 4)
    assert "deviations_t" not in fn.slots and fn.method == 0


def test_launcher_rejects_channels_before_device_calls():
    from katsdpsigproc_amd import _lib, build_native

    if not os.path.exists(_lib.LIB_PATH):
        build_native.build()
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    for channels in (262145, 10**6):
        rc = lib.ksp_madnz_t(0, None, buf, buf, channels, 1, channels)
        assert rc != 0
        assert str(channels) in _lib.last_error() and "1..262144" in _lib.last_error()


@pytest.mark.parametrize("channels, baselines", [(32768, 8), (262144, 2)])
def test_golden_noise(channels, baselines, long_golden):
    """The oracle and the host class both reproduce the reference on long rows."""
    from katsdpsigproc_amd.rfi import host
    from oracle import rfi_oracle as oracle

    dev = inputs_long.noise_long_case(channels, baselines)
    expected = long_golden[f"noise_{channels}x{baselines}"]
    assert expected.dtype == np.float64 and np.all(np.isfinite(expected))
    for est in (oracle.NoiseEstMADHost(), host.NoiseEstMADHost()):
        np.testing.assert_array_equal(est(dev), expected)


def test_golden_flagger(long_golden):
    from katsdpsigproc_amd.rfi import host
    from oracle import rfi_oracle as oracle

    vis, in_flags = inputs_long.flagger_long_case()
    for mod in (oracle, host):
        flagger = mod.FlaggerHost(mod.BackgroundMedianFilterHost(13), mod.NoiseEstMADHost(),
                                  mod.ThresholdSumHost(11.0))  # fmt: skip
        for key, args in (("flagger_32768_none", ()), ("flagger_32768_full", (in_flags,))):
            flags = flagger(vis, *args)
            assert flags.any()
            np.testing.assert_array_equal(np.packbits(flags.astype(np.bool_)), long_golden[key])
