"""The persistent ring kernel's stream phase computes |z| one chunk of four steps ahead of the
median, and chunk 0 of a strip at the end of the strip before it; a workgroup's last strip runs
a second copy of the phase that reads nothing ahead. Flags and noise are compared with the CPU
oracle for exact equality at the shapes that take each of those ways, on noise and with special
values (zero, subnormal, overflowing, infinite, NaN) at the places the change moved: the first
and the last chunk of a lane's run of 64 channels, in the strips on either side of a boundary.

Width 13, 11 sigma, 4 windows, 4096 channels; the noise is ``generate_data`` of the reference's
scripts/rfiflagtest.py (``synth_block`` of bench.py)."""

import numpy as np
import pytest

from tests import inputs

pytestmark = pytest.mark.gpu

CHANNELS = 4096
RUN = 64  # channels per lane
# 8: one strip, a workgroup's first and last at once. 2060: 257 strips for 256 workgroups that
# each take two to begin with, so about half of them run one strip that is followed by another
# and then their last; the 4 left over go to the 4-baseline kernel. 4104: 513 strips, two or
# three per workgroup.
SHAPES = [8, 2060, 4104]

SPECIALS = [
    np.complex64(0),
    np.complex64(complex(1e-40, 1e-41)),  # subnormal
    np.complex64(complex(3e38, 3e38)),  # finite, |z| overflows
    np.complex64(complex(np.inf, 0.0)),
    np.complex64(complex(np.nan, 0.0)),
]
# position in a lane's run: chunk 0 (converted across the strip boundary) at both ends, the
# first step of chunk 1, the last chunk at both ends
OFFSETS = [0, 3, 4, 60, 63]


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

    rfi_oracle.set_threads(rfi_oracle.max_threads())
    yield rfi_oracle
    rfi_oracle.set_threads(1)


@pytest.fixture(scope="module")
def noise_block():
    """The largest shape's noise, generated once; the smaller shapes are its first baselines.
    Tests copy what they change."""
    vis = inputs.generate_data(CHANNELS, max(SHAPES), seed=5)
    vis.setflags(write=False)
    return vis


def special_baselines(baselines):
    """Whole strips of 8 baselines at the start, in the middle and at the end of the strips the
    ring kernel takes, strips of even and odd number next to each other: with the strips handed
    out two at a time, both first and later strips of a workgroup, and every chosen baseline
    has chosen neighbours, across strip boundaries too."""
    n_strips = baselines // 8
    strips = [0, 1, 2, 3, n_strips // 2, n_strips // 2 + 1, n_strips - 2, n_strips - 1]
    return [8 * s + w for s in strips for w in range(8)]


def plant_specials(vis):
    """One special visibility in each chosen baseline: every value at every offset, in the first,
    the last and other lanes."""
    chosen = special_baselines(vis.shape[1])
    assert len(set(chosen)) == len(chosen) >= 2 * len(SPECIALS) * len(OFFSETS)
    for j, b in enumerate(chosen):
        combo = j % (len(SPECIALS) * len(OFFSETS))
        value = SPECIALS[combo % len(SPECIALS)]
        offset = OFFSETS[combo // len(SPECIALS)]
        lane = (0, 63)[j % 2] if j % 5 == 0 else (11 * j + 1) % 64
        vis[RUN * lane + offset, b] = value


def run_ring(context, queue, vis):
    """The flagger without the deviations output, ring kernel forced; twice, because the second
    launch finds the scheduling counters as the first left them."""
    from katsdpsigproc_amd import _lib
    from katsdpsigproc_amd.rfi import device

    template = device.FlaggerDeviceTemplate(
        device.BackgroundMedianFilterDeviceTemplate(context, 13),
        device.NoiseEstMADTDeviceTemplate(context, 10240),
        device.ThresholdSumDeviceTemplate(context, 4),
        keep_deviations=False,
    )
    fn = template.instantiate(queue, *vis.shape, threshold_args={"n_sigma": 11.0})
    assert isinstance(fn, device.FusedFlaggerDevice)
    fn.ensure_all_bound()
    fn.buffer("vis").set(queue, vis)
    outs = []
    for _ in range(2):
        fn.buffer("flags").set(queue, np.full(vis.shape, 255, np.uint8))
        with _lib.fused_ring_mode(1):
            fn()
        path = _lib.call("ksp_flagger_fused_last_path")
        assert path & _lib.FUSED_PATH_RING, f"expected the ring kernel, last path = {path}"
        assert bool(path & _lib.FUSED_PATH_STRIP) == bool(vis.shape[1] % 8), path
        outs.append((fn.buffer("flags").get(queue), fn.buffer("noise").get(queue)))
    return outs


def check(context, queue, oracle, vis):
    with np.errstate(all="ignore"):
        ref_flags, ref_noise = oracle.flagger_full(vis, width=13, n_sigma=11.0, n_windows=4)
    for flags, noise in run_ring(context, queue, vis):
        np.testing.assert_array_equal(ref_noise.astype(np.float32), noise)
        np.testing.assert_array_equal(ref_flags, flags)


@pytest.mark.parametrize("baselines", SHAPES)
def test_noise(baselines, context, command_queue, oracle, noise_block):
    check(context, command_queue, oracle, np.ascontiguousarray(noise_block[:, :baselines]))


@pytest.mark.parametrize("baselines", SHAPES[1:])
def test_special_values(baselines, context, command_queue, oracle, noise_block):
    vis = np.array(noise_block[:, :baselines])
    plant_specials(vis)
    # (the specials are there, one per chosen baseline, and nowhere else)
    odd = ~np.isfinite(vis) | (vis == 0) | (np.abs(vis.real) > 1e38) | (np.abs(vis.real) < 1e-38)
    assert np.array_equal(np.flatnonzero(odd.sum(axis=0) == 1), np.sort(special_baselines(baselines)))
    assert int(odd.sum()) == len(special_baselines(baselines))
    check(context, command_queue, oracle, vis)
