"""Wide median windows (odd widths 33 to 255) without a GPU: template wiring, the golden
vectors of the reference against the oracle and the host classes, and the launcher's
width check."""

import ctypes
import hashlib
import os

import numpy as np
import pytest

from tests import inputs
from tests.fakes import FakeContext

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (33, 63, 127, 255)
MODES = ("none", "channel", "full")


@pytest.fixture(scope="module")
def wide_golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "rfi_host_wide_golden.npz"),
                   allow_pickle=False)  # fmt: skip


def digest(a):
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        a = a + 0.0
    return hashlib.sha256(a.tobytes()).hexdigest()


def test_wide_templates_wire_up():
    from katsdpsigproc_amd.rfi import device

    ctx = FakeContext()
    queue = ctx.create_command_queue()
    for width in (33, 255):
        t = device.BackgroundMedianFilterDeviceTemplate(
            ctx, width, use_flags=device.BackgroundFlags.FULL, tuning={"wgs": 64, "csplit": 4}
        )
        op = t.instantiate(queue, 100, 10)
        op.ensure_all_bound()
        op()
        name, args = queue.launches[-1]
        assert name == "ksp_background_median_filter"
        assert int(args[7]) == width and int(args[9]) == device.BackgroundFlags.FULL.value
        assert int(args[10]) == 4
    for width in (257, 34, 256, 1):
        with pytest.raises(ValueError, match="3..255"):
            device.BackgroundMedianFilterDeviceTemplate(ctx, width)


def test_wide_flagger_is_the_sequence():
    from katsdpsigproc_amd.rfi import device

    ctx = FakeContext()
    queue = ctx.create_command_queue()

    def template(fused=None):
        return device.FlaggerDeviceTemplate(
            device.BackgroundMedianFilterDeviceTemplate(ctx, 63),
            device.NoiseEstMADTDeviceTemplate(ctx, 10240),
            device.ThresholdSumDeviceTemplate(ctx),
            fused=fused,
        )

    assert not template().fusable(4096)
    fn = template().instantiate(queue, 4096, 16, threshold_args={"n_sigma": 11.0})
    assert isinstance(fn, device.FlaggerDevice)
    with pytest.raises(ValueError):
        template(fused=True).instantiate(queue, 4096, 16)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("amplitudes", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_golden_background(width, amplitudes, mode, wide_golden):
    """The oracle and the host class both reproduce the reference bit for bit."""
    from katsdpsigproc_amd.rfi import host
    from oracle import rfi_oracle as oracle

    vis_big, flags_big = inputs.background_case()
    vis = oracle.abs_c64(vis_big) if amplitudes else vis_big
    flags = {"none": None, "channel": flags_big[:, 0], "full": flags_big}[mode]
    key = f"background_w{width}_{'amp' if amplitudes else 'cplx'}_{mode}"
    for bg in (oracle.BackgroundMedianFilterHost(width, amplitudes),
               host.BackgroundMedianFilterHost(width, amplitudes)):  # fmt: skip
        dev = bg(vis) if flags is None else bg(vis, flags)
        np.testing.assert_array_equal(dev[:, inputs.BACKGROUND_COLS], wide_golden[key + "_cols"])
        assert digest(dev) == str(wide_golden[key + "_sha"])


def test_golden_narrow_band(wide_golden):
    from katsdpsigproc_amd.rfi import host
    from oracle import rfi_oracle as oracle

    vis_big, flags_big = inputs.background_case()
    key = "background_w255_narrow_cplx_full"
    for bg in (oracle.BackgroundMedianFilterHost(255), host.BackgroundMedianFilterHost(255)):
        dev = bg(vis_big[:100], flags_big[:100])
        np.testing.assert_array_equal(dev[:, inputs.BACKGROUND_COLS], wide_golden[key + "_cols"])
        assert digest(dev) == str(wide_golden[key + "_sha"])


def test_golden_flagger(wide_golden):
    from katsdpsigproc_amd.rfi import host
    from oracle import rfi_oracle as oracle

    vis, _spikes, in_flags = inputs.flagger_case()
    for mod in (oracle, host):
        flagger = mod.FlaggerHost(mod.BackgroundMedianFilterHost(63), mod.NoiseEstMADHost(),
                                  mod.ThresholdSumHost(11.0))  # fmt: skip
        for key, args in (("flagger_w63_sum_none", ()), ("flagger_w63_sum_full", (in_flags,))):
            flags = flagger(vis, *args)
            np.testing.assert_array_equal(np.packbits(flags.astype(np.bool_)), wide_golden[key])


def test_launcher_rejects_width_before_device_calls():
    from katsdpsigproc_amd import _lib, build_native

    if not os.path.exists(_lib.LIB_PATH):
        build_native.build()
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    flags = (ctypes.c_uint8 * 64)()
    for width in (257, 601, 34, 1):
        rc = lib.ksp_background_median_filter(0, None, buf, buf, flags, 8, 8, 8, 8, width, 0, 0, 0)
        assert rc != 0
        assert str(width) in _lib.last_error() and "3..255" in _lib.last_error()
