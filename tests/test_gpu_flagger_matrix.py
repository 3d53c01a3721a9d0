"""Every case of tests/flagger_matrix.py on the GPU: the template built as a user builds it,
whatever flagger ``instantiate`` returns, run twice, against the oracle. The fused kernels are
held to ``oracle.flagger_full`` exactly (the bar of tests/test_gpu_flagger.py), the
kernel-per-stage sequence to the oracle's stages chained through float32 intermediates
(``test_sequence_sum_matches_staged_oracle``). tests/test_flagger_matrix.py proves, without a
GPU, that the table covers every pair of option levels and that every case has something to
find."""

import numpy as np
import pytest

from tests import flagger_matrix as fm
from tests import subviews

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def context():
    from katsdpsigproc_amd import accel

    return accel.create_some_context(interactive=False)


@pytest.fixture(scope="module")
def command_queue(context):
    return context.create_command_queue()


def build_template(context, case):
    from katsdpsigproc_amd.rfi import device

    bg = device.BackgroundMedianFilterDeviceTemplate(
        context, case.width, is_amplitude=case.amplitudes,
        use_flags=device.BackgroundFlags[case.mask])  # fmt: skip
    if case.noise_transposed:
        ne = device.NoiseEstMADTDeviceTemplate(context, fm.MADT_MAX_CHANNELS)
    else:
        ne = device.NoiseEstMADDeviceTemplate(context)
    if case.sum_threshold:
        th = device.ThresholdSumDeviceTemplate(context, n_windows=case.n_windows,
                                               flag_value=case.flag_value,
                                               transposed=case.threshold_transposed)  # fmt: skip
    else:
        th = device.ThresholdSimpleDeviceTemplate(context, case.threshold_transposed,
                                                  flag_value=case.flag_value)  # fmt: skip
    return device.FlaggerDeviceTemplate(
        bg, ne, th, fused=False if case.forced_sequence else None,
        keep_deviations=case.keep_deviations, tuning={"vis_pad": case.vis_pad})  # fmt: skip


def pad_rows(fn, name, extra):
    """At least `extra` more elements in every row of slot `name` (if the flagger has it), as a
    caller asks for them: through a linked Dimension, before anything is bound."""
    from katsdpsigproc_amd import accel

    slot = fn.slots.get(name)
    if slot is not None:
        dim = slot.dimensions[-1]
        dim.link(accel.Dimension(dim.size, min_padded_size=dim.size + extra))


def upload(command_queue, buffer, data=None, inside=None):
    """`data` into `buffer` with poison (NaN, or bytes of 0xFF) in the padding of its rows; or,
    for an output, sentinel bytes in the padding and `inside` (a byte value; default the
    sentinel as well) in the rows."""
    from katsdpsigproc_amd import accel

    host = buffer.empty_like()
    padded = accel.HostArray.padded_view(host)
    if data is not None:
        padded[...] = subviews.poison_array(padded.size, buffer.dtype).reshape(padded.shape)
        host[...] = data
    else:
        padded[...] = subviews.sentinel_array(padded.shape, buffer.dtype)
        if inside is not None:
            host[...] = inside
    buffer.set(command_queue, host)


def download(command_queue, buffer, name):
    """The rows of an output; every byte of their padding must still hold the sentinel."""
    from katsdpsigproc_amd import accel

    host = buffer.get(command_queue)
    padded = accel.HostArray.padded_view(host)
    outside = np.ones(padded.shape, bool)
    outside[tuple(slice(0, n) for n in buffer.shape)] = False
    expected = subviews.sentinel_array(padded.shape, buffer.dtype)
    damaged = outside & (padded.view(np.uint8).reshape(padded.shape + (-1,))
                         != expected.view(np.uint8).reshape(padded.shape + (-1,))).any(axis=-1)
    assert not damaged.any(), (
        f"{name}: {int(damaged.sum())} padding elements of a buffer of shape {buffer.shape} in "
        f"{buffer.padded_shape} were written, the first at {tuple(np.argwhere(damaged)[0])}")
    return np.array(host)


def prepare(fn, case, command_queue, fused):
    """Pad, bind and upload. `vis_pad` reaches the fused flagger through the template's tuning
    and the sequence through a linked Dimension; with it, the rows of the other 2-D slots get
    a few elements as well (odd strides), so that their padding exists and is checked."""
    if case.vis_pad:
        if not fused:
            pad_rows(fn, "vis", case.vis_pad)
        pad_rows(fn, "flags", 5)
        pad_rows(fn, "deviations", 3)
        if case.mask == "FULL":
            pad_rows(fn, "input_flags", 7)
    fn.ensure_all_bound()
    vis = fn.buffer("vis")
    assert vis.padded_shape[1] >= case.baselines + case.vis_pad
    upload(command_queue, vis, fm.make_input(case))
    if case.mask != "NONE":
        upload(command_queue, fn.buffer("input_flags"), fm.make_mask(case))


def expected_path(case, mode):
    """KSP_FUSED_PATH_* bits of a fused launch, from the documented conditions."""
    from katsdpsigproc_amd import _lib

    if case.channels > 4096:
        return _lib.FUSED_PATH_LONG
    if mode == 1 and fm.ring_eligible(case):
        return _lib.FUSED_PATH_RING | (_lib.FUSED_PATH_STRIP if case.baselines % 8 else 0)
    return _lib.FUSED_PATH_STRIP


def check_fused(fn, case, command_queue):
    from katsdpsigproc_amd import _lib

    with np.errstate(all="ignore"):
        ref_flags, ref_noise, ref_dev = fm.reference(case)
        ref_noise, ref_dev = ref_noise.astype(np.float32), ref_dev.astype(np.float32)
    assert fn.slots["deviations"].is_bound() == case.keep_deviations
    counters = fn._workspace.get(command_queue).copy()
    for mode in (-1, 1):
        for _ in range(2):
            upload(command_queue, fn.buffer("flags"), inside=255)
            upload(command_queue, fn.buffer("noise"))
            if case.keep_deviations:
                upload(command_queue, fn.buffer("deviations"))
            with _lib.fused_ring_mode(mode):
                fn()
            path = _lib.call("ksp_flagger_fused_last_path")
            assert path == expected_path(case, mode), f"ring mode {mode}: last path = {path}"
            flags = download(command_queue, fn.buffer("flags"), "flags")
            np.testing.assert_array_equal(ref_noise, fn.buffer("noise").get(command_queue))
            if case.keep_deviations:
                dev = download(command_queue, fn.buffer("deviations"), "deviations")
                np.testing.assert_array_equal(ref_dev, dev)
            np.testing.assert_array_equal(ref_flags, flags)
            # the scheduling counters are left as they were found
            np.testing.assert_array_equal(counters, fn._workspace.get(command_queue))
    assert not fn.slots["deviations_t"].is_bound() and not fn.slots["flags_t"].is_bound()


def check_sequence(fn, case, command_queue):
    ref_flags, ref_noise, ref_dev = fm.staged_reference(case)
    transposed = case.noise_transposed or case.threshold_transposed
    assert ("deviations_t" in fn.slots) == transposed
    assert ("flags_t" in fn.slots) == case.threshold_transposed
    for _ in range(2):
        upload(command_queue, fn.buffer("flags"), inside=255)
        upload(command_queue, fn.buffer("deviations"))
        upload(command_queue, fn.buffer("noise"))
        fn()
        dev = download(command_queue, fn.buffer("deviations"), "deviations")
        flags = download(command_queue, fn.buffer("flags"), "flags")
        np.testing.assert_array_equal(ref_dev, dev)
        if transposed:
            np.testing.assert_array_equal(ref_dev.T, fn.buffer("deviations_t").get(command_queue))
        np.testing.assert_array_equal(ref_noise, fn.buffer("noise").get(command_queue))
        if case.threshold_transposed:
            np.testing.assert_array_equal(ref_flags.T, fn.buffer("flags_t").get(command_queue))
        np.testing.assert_array_equal(ref_flags, flags)


@pytest.mark.parametrize("case", fm.CASES, ids=[case.id for case in fm.CASES])
def test_case(case, context, command_queue):
    from katsdpsigproc_amd.rfi import device

    template = build_template(context, case)
    threshold_args = {"n_sigma": case.n_sigma}
    if case.sum_threshold:
        threshold_args["threshold_falloff"] = case.threshold_falloff
    fn = template.instantiate(command_queue, case.channels, case.baselines,
                              threshold_args=threshold_args)  # fmt: skip
    # which class came back
    assert template.fusable(case.channels) == fm.documented_fusable(case)
    if case.forced_sequence:
        assert isinstance(fn, device.FlaggerDevice)
    else:
        assert isinstance(fn, device.FusedFlaggerDevice) == template.fusable(case.channels)
    fused = isinstance(fn, device.FusedFlaggerDevice)
    assert fused or isinstance(fn, device.FlaggerDevice)
    assert fused == fm.runs_fused(case)
    print(f"flagger matrix: {fm.kernel_class(case)} <- {case.id}")
    prepare(fn, case, command_queue, fused)
    if fused:
        check_fused(fn, case, command_queue)
    else:
        check_sequence(fn, case, command_queue)
