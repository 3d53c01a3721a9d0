"""Inputs and launch geometry for the tests of the standalone background kernel
(csrc/background.hip): bands whose baselines cover the data that can upset a median, the
masks that go with them, and the shapes at which the kernel's two arithmetic paths meet.

``background_kernel<WIDTH>`` gives a wavefront one channel segment of 64 adjacent baselines.
Without input flags and for WIDTH <= 13, a segment whose halo lies wholly inside the band
takes the merging median, and goes back through the sorted window if any sample it read was
NaN or infinite; every other segment takes the sorted window. Which segment does what follows
from ``ksp_background_median_filter_geometry`` (the launcher's own rule) and
:func:`segment_merges`. Nothing here needs a GPU.
"""

import ctypes

import numpy as np

from tests import inputs

MERGE_WIDTHS = (3, 5, 7, 9, 11, 13)
ALL_WIDTHS = tuple(range(3, 32, 2))
#: one full and one ragged wave column
SWEEP_BASELINES = 65
MODES = ("NONE", "CHANNEL", "FULL")

CONSTANT_BASELINE = 1
ZERO_BASELINE = 5
N_FAMILIES = 4


# ------------------------------------------------------------------------------- geometry
def geometry(channels, baselines, width, csplit):
    """(seg_len, n_segs) of the launch, from the launcher's own rule."""
    from katsdpsigproc_amd import _lib

    seg_len, n_segs = ctypes.c_int(-1), ctypes.c_int(-1)
    _lib.call("ksp_background_median_filter_geometry", channels, baselines, width, csplit,
              ctypes.byref(seg_len), ctypes.byref(n_segs))  # fmt: skip
    return seg_len.value, n_segs.value


def segments(channels, seg_len, n_segs):
    """[(c_begin, c_end)] of every segment."""
    return [(i * seg_len, min(channels, (i + 1) * seg_len)) for i in range(n_segs)]


def segment_merges(channels, width, c_begin, c_end):
    """Whether a segment without input flags starts on the merging median (width <= 13)."""
    half = width // 2
    return width <= 13 and c_begin - half >= 0 and c_end + half <= channels


def seam_sweep(width):
    """[(csplit, channels)] of the seam sweep of one width (tests/test_background_segments.py
    asserts what it covers)."""
    cases = [(3, channels) for channels in range(8 * width + 1, 16 * width + 3)]
    cases += [(6, channels) for channels in range(20 * width, 26 * width + 7)]
    # segment counts that are multiples of 4 (four segments share a workgroup): 4 and 8
    # segments of the minimum length, 8 with a last one of half - 1 channels, 8 longer ones
    # whole and with a short last one
    half = width // 2
    cases += [(8, 16 * width), (8, 32 * width), (8, 28 * width + max(half - 1, 1)),
              (8, 8 * (4 * width + 3)), (8, 8 * (4 * width + 3) - 5)]  # fmt: skip
    return cases


def seam_sweep_max_channels(width):
    return max(channels for _, channels in seam_sweep(width))


def fallback_shape(width):
    """(channels, baselines, csplit) of the fallback sweep: 5 segments of 4 * width + 3
    channels and one wave column per channel."""
    channels = 5 * (4 * width + 3)
    return channels, 64 * channels, 5


def sorted_window_channels(width):
    """Band lengths of the every-width sweep (csplit 3): three segments of 4 * width channels
    with tails around the halo and the window, then bands shorter than a window."""
    half = width // 2
    tails = (1, half, half + 1, width - 1, width, width + 1, 2 * width, 4 * width)
    return [8 * width + t for t in tails], sorted({1, 2, half, half + 1, width - 1, width, width + 1})


# ---------------------------------------------------------------------------------- bands
def _noise(rs, channels, n):
    """Complex normal noise with sparse strong spikes."""
    z = inputs.complex_normal(rs, (channels, n))
    spikes = rs.random_sample((channels, n)) < 1.0 / 16.0
    amp = rs.random_sample((channels, n)) * 20.0 + 50.0
    return z + spikes * amp * np.exp(2j * np.pi * rs.random_sample((channels, n)))


def _ties(rs, channels, n):
    """Amplitudes from {0, 0.25, 0.5, 0.75}, on either axis of the complex plane."""
    a = rs.randint(0, 4, (channels, n)) * 0.25
    return np.where(rs.random_sample((channels, n)) < 0.5, a, 1j * a)


def _magnitudes(rs, channels, n):
    """Exponents from 2^-149 (denormal) to 2^127: any exponent in even columns, neighbouring
    channels alternating huge and tiny in odd ones. One component only, so that every
    amplitude stays finite."""
    mant = 1.0 + rs.random_sample((channels, n))
    any_exp = rs.randint(-149, 128, (channels, n))
    huge = rs.randint(100, 128, (channels, n))
    tiny = rs.randint(-149, -99, (channels, n))
    alternating = np.where((np.arange(channels) % 2 == 0)[:, None], huge, tiny)
    exponent = np.where((np.arange(n) % 2 == 0)[None, :], any_exp, alternating)
    a = np.ldexp(mant, exponent)
    a[0, :] = np.ldexp(1.0, 127)  # the extremes themselves
    if channels > 1:
        a[1, :] = np.ldexp(1.0, -149)
    return np.where(rs.random_sample((channels, n)) < 0.5, a, 1j * a)


def _lattice(rs, channels, n):
    """Small integers in both components: equal amplitudes from different visibilities."""
    return rs.randint(-3, 4, (channels, n)) + 1j * rs.randint(-3, 4, (channels, n))


def make_band(channels, baselines, kind, seed):
    """channels x baselines of complex64 (`kind` "cplx") or float32 amplitudes ("amp"), every
    amplitude finite. Baseline b belongs to family b % 4: noise with spikes, heavy ties,
    the whole range of magnitudes, and a lattice of small integers; baseline 1 is constant and
    baseline 5 all zero. Amplitude input is signed and holds -0.0: the host class takes any
    float32 there."""
    assert kind in ("cplx", "amp")
    rs = np.random.RandomState(seed)
    band = np.empty((channels, baselines), np.complex128)
    for family, make in enumerate((_noise, _ties, _magnitudes, _lattice)):
        n = len(range(family, baselines, N_FAMILIES))
        band[:, family::N_FAMILIES] = make(rs, channels, n)
    if baselines > CONSTANT_BASELINE:
        band[:, CONSTANT_BASELINE] = 0.375
    if baselines > ZERO_BASELINE:
        band[:, ZERO_BASELINE] = 0.0
    if kind == "cplx":
        return band.astype(np.complex64)
    # one real number per sample: the sum of the components (one of them is zero in the
    # families of ties and magnitudes), with random signs, and -0.0 for some of the zeros
    amp = (band.real + band.imag) * np.where(rs.random_sample(band.shape) < 0.5, -1.0, 1.0)
    amp = amp.astype(np.float32)
    amp[(amp == 0) & (rs.random_sample(amp.shape) < 0.5)] = -0.0
    return amp


def make_noise(channels, baselines, kind, seed):
    """A clean band: complex normal noise, or signed normal amplitudes."""
    rs = np.random.RandomState(seed)
    re = rs.standard_normal((channels, baselines)).astype(np.float32)
    if kind == "amp":
        return re
    out = np.empty((channels, baselines), np.complex64)
    out.real = re
    out.imag = rs.standard_normal((channels, baselines)).astype(np.float32)
    return out


def make_masks(channels, baselines, width, seed):
    """(channel mask, per-sample mask), uint8 with any non-zero value for a flag, both about
    10 % flagged; the per-sample mask holds one block of width + 2 channels (from channel 2,
    baselines 3 .. 39) without a single valid sample."""
    rs = np.random.RandomState(seed)
    chan = np.where(rs.random_sample(channels) < 0.1, rs.randint(1, 256, channels), 0)
    full = np.where(rs.random_sample((channels, baselines)) < 0.1,
                    rs.randint(1, 256, (channels, baselines)), 0)  # fmt: skip
    full[2 : 2 + width + 2, 3:40] = 4
    return chan.astype(np.uint8), full.astype(np.uint8)


def mode_flags(mode, chan, full, channels):
    """The flags argument of a mode for the first `channels` channels."""
    return {"NONE": None, "CHANNEL": chan[:channels], "FULL": full[:channels]}[mode]


# ------------------------------------------------------------------------ non-finite plants
def nonfinite_values(kind):
    """The values a sample can hold that take no part in a window: NaN and +inf, and for
    amplitude input -inf as well."""
    return (np.nan, np.inf) if kind == "cplx" else (np.nan, np.inf, -np.inf)


def plant_positions(channels):
    """(channel, baseline) of the fallback sweep's plants: wave column k carries exactly one,
    at channel k, in baseline 64 k + (k mod 64)."""
    k = np.arange(channels)
    return k, 64 * k + k % 64


def plant(band, rows, cols, value):
    """`band` with `value` at (rows, cols), modified in place; a complex sample gets it in one
    component (the imaginary one in odd rows)."""
    if band.dtype == np.complex64:
        rows, cols = np.asarray(rows), np.asarray(cols)
        band[rows, cols] = np.where(rows % 2 == 0, complex(value, 0.5), complex(0.5, value))
    else:
        band[rows, cols] = value
    return band


def scatter_plants(band, kind, seed):
    """A copy of `band` with about 3 % of its samples NaN or infinite, alone and in runs."""
    rs = np.random.RandomState(seed)
    out = band.copy()
    values = nonfinite_values(kind)
    pick = rs.randint(0, len(values), band.shape)
    hit = rs.random_sample(band.shape) < 0.03
    hit[1:] |= hit[:-1] & (rs.random_sample((band.shape[0] - 1, band.shape[1])) < 0.3)
    for i, value in enumerate(values):
        rows, cols = np.nonzero(hit & (pick == i))
        plant(out, rows, cols, value)
    return out
