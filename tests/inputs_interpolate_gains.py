"""Seeded inputs for the tests of ``rfi.host.InterpolateGainsHost`` and of the device operation
(tests/test_interpolate_gains.py, tests/test_gpu_interpolate_gains.py): gains of several kinds,
one kind per input, with the delay model, the band-wide gains and the status that go with them,
the smooth bandpass of the accuracy tests, and the comparison both files use."""

import numpy as np

from tests.inputs_fit_delays import make_status

f32 = np.float32

#: the kinds of input that :func:`make_case` deals out, input ``p`` getting kind
#: ``KINDS[(p + first) % len(KINDS)]``
KINDS = (
    "all_kept",
    "random_holes",  # about 25 % of the channels NaN, one by one
    "none_kept",
    "one_kept",  # every channel but one NaN
    "first_only",  # only channel 0 kept
    "last_only",  # only the last channel kept
    "alternating",  # kept, missing, kept, ...
    "gap_exact",  # gaps of exactly max_gap channels across every seam of the kernel
    "gap_over",  # gaps of max_gap + 1 channels there
    "parts",  # +inf, -inf and NaN in one part only, the other part finite
    "ends",  # max_gap channels missing at the start, max_gap + 1 at the end
    "bad_model",  # model entries that are not finite, on kept and on missing channels
    "huge",  # magnitudes of 3e38: products and differences overflow
    "zeros",  # +0 and -0: nothing to normalise by
    "runs",  # runs of 1 .. 2 max_gap + 2 missing channels
    "ends_over",  # max_gap + 1 channels missing at the start, max_gap at the end
)


def threads_of(channels):
    """The threads of the workgroup of csrc/interpolate_gains.hip for a band of `channels`: the
    next power of two, at least 64 and at most 1024."""
    c_pad = 1
    while c_pad < channels:
        c_pad *= 2
    return min(max(c_pad, 64), 1024)


def seams(channels):
    """The channels in front of which the kernel changes hands: the second wavefront's first
    channel, the first channel of a thread's second round (a whole workgroup on), and the first
    channel whose word of `kept` bits is scanned by the second wavefront."""
    return sorted({c for c in (64, threads_of(channels), 4096) if c < channels})


def bandpass(channels, period=1024.0):
    """complex128 (channels,): amplitude ``1 + 0.2 cos(2 pi c / period)``, phase
    ``0.3 sin(2 pi c / period)``."""
    theta = 2 * np.pi * np.arange(channels) / period
    return (1 + 0.2 * np.cos(theta)) * np.exp(0.3j * np.sin(theta))


def bandpass_curvature(period=1024.0):
    """The largest ``|f''(c)|`` of :func:`bandpass`, from its formula on a grid of an eighth of
    a channel over one period."""
    theta = 2 * np.pi * np.arange(0, period, 0.125) / period
    w = 2 * np.pi / period
    a, a1, a2 = 1 + 0.2 * np.cos(theta), -0.2 * w * np.sin(theta), -0.2 * w * w * np.cos(theta)
    p1, p2 = 0.3 * w * np.cos(theta), -0.3 * w * w * np.sin(theta)
    return float(np.abs(a2 + 2j * a1 * p1 + 1j * a * p2 - a * p1 * p1).max())


def punch(column, start, length):
    """NaN in `length` channels of `column` from `start` on (clipped to the band)."""
    column[max(start, 0) : max(start + length, 0)] = complex(np.nan, np.nan)


def make_column(rs, kind, channels, max_gap):
    """(gains complex64 (channels,), model complex64 (channels,)) for one input of `kind`."""
    amplitude = np.exp2(rs.uniform(-3, 3))
    nu = rs.uniform(-0.3, 0.3)
    c = np.arange(channels)
    rotation = np.exp(2j * np.pi * (c * nu + rs.uniform()))
    noise = 0.02 * (rs.standard_normal(channels) + 1j * rs.standard_normal(channels))
    smooth = amplitude * (bandpass(channels, rs.uniform(200, 2000)) + noise)
    column = smooth * rotation
    model = rotation.astype(np.complex64)
    if kind == "random_holes":
        column[rs.random_sample(channels) < 0.25] = np.nan
    elif kind == "none_kept":
        column[:] = complex(np.nan, 1.0)
    elif kind in ("one_kept", "first_only", "last_only"):
        at = {"one_kept": rs.randint(channels), "first_only": 0, "last_only": channels - 1}[kind]
        value = column[at]
        column[:] = complex(1.0, np.nan)
        column[at] = value
    elif kind == "alternating":
        column[(c + rs.randint(2)) % 2 == 1] = np.nan
    elif kind in ("gap_exact", "gap_over"):
        length = max_gap + (kind == "gap_over")
        free = 1  # the first channel a gap may take: one kept channel lies in front of it
        for seam in seams(channels):
            start = seam - (length + 1) // 2
            if start >= free and start + length < channels:
                punch(column, start, length)
                free = start + length + 1
    elif kind in ("ends", "ends_over"):
        at_start = max_gap + (kind == "ends_over")
        at_end = max_gap + (kind == "ends")
        if at_start + at_end < channels:
            punch(column, 0, at_start)
            punch(column, channels - at_end, at_end)
    elif kind == "huge":
        column = column * (3e38 / amplitude)
        column[rs.random_sample(channels) < 0.1] = np.nan
    elif kind == "zeros":
        column = np.where(rs.random_sample(channels) < 0.5, 0.0, -0.0) + 1j * np.where(
            rs.random_sample(channels) < 0.5, 0.0, -0.0)  # fmt: skip
        column[rs.random_sample(channels) < 0.1] = np.nan
    elif kind == "runs":
        at = rs.randint(0, 3)
        while at < channels:
            length = rs.randint(1, 2 * max_gap + 3)
            punch(column, at, length)
            at += length + rs.randint(1, 6)
    with np.errstate(over="ignore"):  # (huge: some parts become infinite)
        column = column.astype(np.complex64)
    if kind == "parts":
        where = rs.random_sample(channels)
        column.real[where < 0.05] = np.inf
        column.imag[(where >= 0.05) & (where < 0.1)] = -np.inf
        column.real[(where >= 0.1) & (where < 0.15)] = np.nan
        column.imag[(where >= 0.15) & (where < 0.2)] = np.nan
    elif kind == "bad_model":
        column[rs.random_sample(channels) < 0.2] = np.nan
        where = rs.random_sample(channels)
        model.real[where < 0.05] = np.inf
        model.imag[(where >= 0.05) & (where < 0.1)] = np.nan
        model[(where >= 0.1) & (where < 0.15)] = complex(-np.inf, np.nan)
    return column, model


def make_case(seed, channels, n_inputs, max_gap, first=0, mask=0x0F, kinds=KINDS):
    """(gains, status, model, scale, kinds per input): complex64 (channels, n_inputs), uint8
    (channels,), complex64 (channels, n_inputs), complex64 (n_inputs,). One scale in eight is
    NaN and one is zero."""
    rs = np.random.RandomState(seed)
    gains = np.empty((channels, n_inputs), np.complex64)
    model = np.empty((channels, n_inputs), np.complex64)
    names = []
    for p in range(n_inputs):
        kind = kinds[(p + first) % len(kinds)]
        gains[:, p], model[:, p] = make_column(rs, kind, channels, max_gap)
        names.append(kind)
    scale = (np.exp2(rs.uniform(-2, 2, n_inputs)) * np.exp(2j * np.pi * rs.uniform(size=n_inputs)))
    scale = scale.astype(np.complex64)
    lot = rs.randint(0, 8, n_inputs)
    scale[lot == 0] = complex(np.nan, 1.0)
    scale[lot == 1] = 0
    status = make_status(seed + 1, channels, mask)
    return gains, status, model, scale, names


def assert_same(want, got, what=""):
    """Same dtype, shape and bit patterns; the one exception is a float (or a part of a
    complex number) that is NaN in `want`, which has to be a NaN in `got`."""
    assert want.dtype == got.dtype and want.shape == got.shape, what
    want, got = np.ascontiguousarray(want), np.ascontiguousarray(got)
    if want.dtype.kind in "iu":
        nan = np.zeros(want.shape, bool)
        words_want, words_got, parts_got = want, got, got
    else:
        parts_want, parts_got = want.view(f32), got.view(f32)
        words_want, words_got = want.view(np.uint32), got.view(np.uint32)
        nan = np.isnan(parts_want)
    bad = np.where(nan, ~np.isnan(parts_got), words_want != words_got)
    assert not bad.any(), (
        f"{what}: {np.count_nonzero(bad)} of {bad.size} words differ, first at "
        f"{np.argwhere(bad)[0]}: want {words_want[bad][0]:#x}, got {words_got[bad][0]:#x}")  # fmt: skip
