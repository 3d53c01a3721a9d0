"""The two rarely taken ends of the fused flagger's MAD (``mad_noise`` of csrc/fused_common.h),
on inputs that are known to reach them.

Branch 1: the count of non-zero deviations is even and the upper median is the smallest sample
of its key bin, so the lower median is the largest value BELOW the bin -- found in one pass
over the float32 patterns, with the samples at that value recomputed exactly unless all of them
are exact as float32. Branch 2 (ring kernel only): the bin's candidates are ranked on their
float32 patterns, and the exact float64 values are recomputed only when an inexact candidate
sits at the pattern of rank r (or r - 1 for an even count).

Every input is classified here on the CPU first -- the oracle's float64 deviations, ``d32 =
float32(|dev|)``, a sample exact iff ``float64(d32) == |dev|``, the kernel's 15-bit key
``(pattern + 0xffff) >> 16`` -- and the test asserts that the class it is there for is present
before it looks at the GPU: an input that stops reaching a branch fails instead of passing for
nothing. Then flags and noise of two launches are compared with the oracle for exact equality,
through the ring kernel and the 4-baseline kernel at 4096 channels (64 channels per lane) and
through the 4-baseline kernels at 1024 and 2048 channels (16 and 32 per lane).

Width 13, 11 sigma, 4 windows, 512 baselines."""

import numpy as np
import pytest

from tests import inputs

pytestmark = pytest.mark.gpu

CHANNELS = 4096
BASELINES = 512
WIDTH = 13
LIST_CAP = 64  # bins of up to 64 samples are ranked one per lane (step 3a)

# (channels, ring mode): the ring kernel, and the 4-baseline kernels with 64, 16 and 32
# channels per lane
MODES = [(4096, 1), (4096, 0), (1024, 0), (2048, 0)]
D_SEED = 1  # ties_inexact: gives 6 baselines of class d (counted on the CPU)


def noise():
    return inputs.generate_data(CHANNELS, BASELINES, seed=5)


def spread():
    """Class B: every sample scaled by its own log-normal factor. The amplitudes of a window
    then span several binades and most differences round."""
    scale = np.exp(np.random.RandomState(7).normal(0.0, 1.5, (CHANNELS, BASELINES)))
    return (noise() * scale).astype(np.complex64)


def quantised():
    """Class C: real amplitudes on a grid of 1/512. Every deviation is exact, many are equal."""
    return (np.round(noise().real * 512.0) / 512.0).astype(np.complex64)


def ties_inexact(seed=D_SEED):
    """Class D: a coarse grid of 1/8 with offsets of 0 .. 3 times 2^-22 added, each sample
    scaled by 1/8, 1 or 8: equal float32 deviations of which some rounded."""
    rs = np.random.RandomState(seed)
    shape = (CHANNELS, BASELINES)
    grid = np.round(noise().real.astype(np.float64) * 8.0) / 8.0
    offs = 2.0 ** -22 * rs.randint(0, 4, shape)
    scale = 2.0 ** rs.choice([-3, 0, 3], shape)
    return ((grid + offs) * scale).astype(np.float32).astype(np.complex64)


def rfi():
    """Class E, second input: the interference of bench.py's ``rfi_variant``."""
    return inputs.add_rfi_sparse(noise(), seed=3)


INPUTS = {"noise": noise, "spread": spread, "quantised": quantised, "ties_inexact": ties_inexact,
          "rfi": rfi}  # fmt: skip


def classify(dev):
    """Per baseline of float64 deviations [channels][baselines], which way the MAD takes.

    Returns a dict of boolean arrays over the baselines:
    ``branch1``  even count and the lower median below the upper median's key bin, at a
                 float32 value that is not zero;
    ``a`` .. ``d``  branch 1 with one sample at the largest float32 value below the bin, exact
                 (a) or not (b), or several of them, all exact (c) or not all (d);
    ``e_needed``, ``e_spared``  the bin holds at most 64 samples of which some are inexact,
                 and one of those does (needed) or none does (spared) have the float32 pattern
                 of rank r or, for an even count with r >= 1, of rank r - 1.
    """
    a = np.abs(dev)
    with np.errstate(over="ignore"):
        d32 = a.astype(np.float32)
    pat = d32.view(np.uint32).astype(np.int64)
    key = (pat + 0xFFFF) >> 16
    exact = d32.astype(np.float64) == a
    names = ("branch1", "a", "b", "c", "d", "e_needed", "e_spared")
    out = {name: np.zeros(dev.shape[1], bool) for name in names}
    for b in range(dev.shape[1]):
        nz = a[:, b] != 0
        n = int(nz.sum())
        if n == 0:
            continue
        order = np.argsort(a[nz, b], kind="stable")
        p, k, ex = pat[nz, b][order], key[nz, b][order], exact[nz, b][order]
        even = n % 2 == 0
        upper = n // 2
        in_bin = np.flatnonzero(k == k[upper])
        r = upper - in_bin[0]  # rank inside the bin (sorted by value, so by key too)
        if even and r == 0 and p[upper - 1] != 0:
            out["branch1"][b] = True
            top = p == p[upper - 1]
            name = ("a" if ex[top].all() else "b") if top.sum() == 1 else \
                   ("c" if ex[top].all() else "d")  # fmt: skip
            out[name][b] = True
        if len(in_bin) <= LIST_CAP and not ex[in_bin].all():
            wanted = [p[upper]] + ([p[upper - 1]] if even and r >= 1 else [])
            needed = bool((np.isin(p[in_bin], wanted) & ~ex[in_bin]).any())
            out["e_needed" if needed else "e_spared"][b] = True
    return out


@pytest.fixture(scope="module")
def context():
    from katsdpsigproc_amd import accel

    return accel.create_some_context(interactive=False)


@pytest.fixture(scope="module")
def command_queue(context):
    return context.create_command_queue()


@pytest.fixture(scope="module")
def cases():
    """name, channels -> (vis, oracle flags, oracle noise as float32, classes); computed on
    first use and shared, read-only, by the tests that follow."""
    from oracle import rfi_oracle

    made = {}
    blocks = {}

    def get(name, channels):
        if (name, channels) not in made:
            if name not in blocks:
                blocks[name] = INPUTS[name]()
            vis = np.ascontiguousarray(blocks[name][:channels])
            rfi_oracle.set_threads(rfi_oracle.max_threads())
            try:
                with np.errstate(all="ignore"):
                    flags, ref_noise, dev = rfi_oracle.flagger_full(
                        vis, width=WIDTH, n_sigma=11.0, n_windows=4, want_deviations=True)
            finally:
                rfi_oracle.set_threads(1)
            case = (vis, flags, ref_noise.astype(np.float32), classify(dev))
            for array in case[:3]:
                array.setflags(write=False)
            made[name, channels] = case
        return made[name, channels]

    return get


def run(context, queue, vis, ring):
    """The flagger without the deviations output, twice (the ring kernel's second launch finds
    the scheduling counters as the first left them)."""
    from katsdpsigproc_amd import _lib
    from katsdpsigproc_amd.rfi import device

    template = device.FlaggerDeviceTemplate(
        device.BackgroundMedianFilterDeviceTemplate(context, WIDTH),
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
        with _lib.fused_ring_mode(ring):
            fn()
        path = _lib.call("ksp_flagger_fused_last_path")
        if ring:
            assert path & _lib.FUSED_PATH_RING, f"expected the ring kernel, last path = {path}"
            assert not path & _lib.FUSED_PATH_STRIP, path
        else:
            assert not path & _lib.FUSED_PATH_RING, f"ring kernel not asked for, last path = {path}"
        outs.append((fn.buffer("flags").get(queue), fn.buffer("noise").get(queue)))
    return outs


def counts(classes):
    return {name: int(hit.sum()) for name, hit in classes.items()}


# What each input is there for, at 4096 channels: class -> fewest baselines.
# (counted on the CPU: noise 30 at branch 1, 28 of them in a; spread 50 and 26 in b, 271
# e_needed and 217 e_spared; quantised 31, all in c; ties_inexact 6 in d with D_SEED; rfi 13
# e_needed and 73 e_spared)
PRESENT = {
    "noise": {"a": 10},
    "spread": {"b": 10, "e_needed": 1, "e_spared": 1},
    "quantised": {"c": 10},
    "ties_inexact": {"d": 1},
    "rfi": {"e_needed": 1, "e_spared": 1},
}
# in the first 1024 and 2048 channels (115 and 73 of the noise's baselines at branch 1, 49 and
# 41 in b, 72 and 52 in c, 1 and 3 in d)
PRESENT_SHORT = {"noise": {"branch1": 10}, "spread": {"b": 10}, "quantised": {"c": 10},
                 "ties_inexact": {"d": 1}}  # fmt: skip


@pytest.mark.parametrize("channels,ring", MODES)
@pytest.mark.parametrize("name", list(INPUTS))
def test_lower_median(name, channels, ring, context, command_queue, cases):
    vis, ref_flags, ref_noise, classes = cases(name, channels)
    found = counts(classes)
    print(f"{name}, {channels} channels: {found}")
    need = PRESENT[name] if channels == CHANNELS else PRESENT_SHORT.get(name, {})
    for cls, fewest in need.items():
        assert found[cls] >= fewest, f"{name} at {channels} channels: class {cls}: {found}"
    for flags, got_noise in run(context, command_queue, vis, ring):
        np.testing.assert_array_equal(ref_noise, got_noise)
        np.testing.assert_array_equal(ref_flags, flags)
