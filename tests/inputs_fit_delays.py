"""Seeded inputs for the tests of ``rfi.host.FitDelaysHost`` and of the device operation
(tests/test_fit_delays.py, tests/test_gpu_fit_delays.py): gains of several kinds, one kind per
input, a status array, a float64 restatement of the estimator and the comparison both use."""

import numpy as np

f32 = np.float32

#: the kinds of input that :func:`make_gains` deals out, input ``p`` getting kind
#: ``KINDS[(p + first) % len(KINDS)]``
KINDS = (
    "tone",  # a exp(2 pi i c nu), nu anywhere in (-0.5, 0.5)
    "zero_delay",  # nu = 0
    "on_bin",  # nu = k / n_fft exactly
    "half_bin",  # nu = (k + 0.5) / n_fft: two neighbouring bins of nearly the same power
    "plus_half",  # nu = +0.5
    "minus_half",  # nu = -0.5
    "noisy",  # amplitude scatter of 30 % and noise of 0.3 per channel
    "missing",  # noisy, with about 10 % of the channels NaN
    "all_nan",
    "one_kept",  # every channel but one NaN
    "two_kept",
    "zeros",  # +0 and -0
    "huge",  # magnitudes of 3e38: the transform overflows, P holds inf and NaN
    "alternating",  # real, 1 0 -1 0 ...: two equal peaks
    "noise",  # no tone at all
    "infinite",  # a tone with infinities and NaN in single parts
    "delta",  # one channel that is not zero: a flat likelihood, den is 0 but for its rounding
    "delta0",  # that channel is channel 0: D1 = D2 = 0 and the step is 0 / 0, always rejected
)


def tone(channels, nu, amplitude=1.0, phase=0.0):
    """complex128 (channels,): ``amplitude exp(i (phase + 2 pi c nu))``."""
    return amplitude * np.exp(1j * (phase + 2 * np.pi * np.arange(channels) * nu))


def make_column(rs, kind, channels, n_fft):
    """(complex64 (channels,), the generating nu or None) for one input of `kind`."""
    amplitude = np.exp2(rs.uniform(-3, 3))
    phase = rs.uniform(-np.pi, np.pi)
    nu = rs.uniform(-0.49, 0.49)
    noise = rs.standard_normal(channels) + 1j * rs.standard_normal(channels)
    if kind == "zero_delay":
        nu = 0.0
    elif kind == "on_bin":
        nu = rs.randint(-n_fft // 2 + 1, n_fft // 2) / n_fft
    elif kind == "half_bin":
        nu = (rs.randint(-n_fft // 2 + 1, n_fft // 2 - 1) + 0.5) / n_fft
    elif kind == "plus_half":
        nu = 0.5
    elif kind == "minus_half":
        nu = -0.5
    column = tone(channels, nu, amplitude, phase)
    if kind in ("noisy", "missing"):
        column *= 1 + 0.3 * rs.standard_normal(channels)
        column += amplitude * 0.3 * np.sqrt(0.5) * noise
    if kind == "missing":
        column[rs.random_sample(channels) < 0.1] = np.nan
    elif kind == "all_nan":
        column[:] = complex(np.nan, np.nan)
        nu = None
    elif kind in ("one_kept", "two_kept"):
        keep = rs.permutation(channels)[: 1 if kind == "one_kept" else 2]
        kept = column[keep]
        column[:] = complex(np.nan, 1.0)
        column[keep] = kept
        nu = None
    elif kind == "zeros":
        column = np.where(rs.random_sample(channels) < 0.5, 0.0, -0.0) + 1j * np.where(
            rs.random_sample(channels) < 0.5, 0.0, -0.0)  # fmt: skip
        nu = None
    elif kind == "huge":
        column = tone(channels, nu, 3e38 * np.sqrt(0.5), phase)
        nu = None
    elif kind == "alternating":
        column = np.array([1, 0, -1, 0] * (channels // 4 + 1), np.complex128)[:channels] * amplitude
        nu = None
    elif kind == "noise":
        column = noise
        nu = None
    elif kind in ("delta", "delta0"):
        at = rs.randint(channels) if kind == "delta" else 0
        value = column[at]
        column = np.zeros(channels, np.complex128)
        column[at] = value
        nu = None
    column = column.astype(np.complex64)
    if kind == "infinite":
        where = rs.random_sample(channels)
        column.real[where < 0.05] = np.inf
        column.imag[(where >= 0.05) & (where < 0.1)] = -np.inf
        column.real[(where >= 0.1) & (where < 0.15)] = np.nan
        nu = None
    return column, nu


def make_gains(seed, channels, n_inputs, n_fft, first=0, kinds=KINDS):
    """(gains complex64 (channels, n_inputs), kinds per input, nu per input as float64 with
    NaN where the kind has no generating tone)."""
    rs = np.random.RandomState(seed)
    gains = np.empty((channels, n_inputs), np.complex64)
    names, nus = [], np.full(n_inputs, np.nan)
    for p in range(n_inputs):
        kind = kinds[(p + first) % len(kinds)]
        gains[:, p], nu = make_column(rs, kind, channels, n_fft)
        names.append(kind)
        if nu is not None:
            nus[p] = nu
    return gains, names, nus


def make_status(seed, channels, mask=0x0F):
    """uint8 (channels,): about 70 % zero, 15 % with bits inside `mask` and 15 % with bits
    outside it only."""
    rs = np.random.RandomState(seed)
    status = np.zeros(channels, np.uint8)
    kind = rs.random_sample(channels)
    inside = [bit for bit in range(8) if mask >> bit & 1]
    outside = [bit for bit in range(8) if not mask >> bit & 1]
    for c in range(channels):
        if kind[c] < 0.15 and inside:
            status[c] = 1 << inside[rs.randint(len(inside))]
            if outside and rs.random_sample() < 0.5:
                status[c] |= 1 << outside[rs.randint(len(outside))]
        elif kind[c] < 0.3 and outside:
            status[c] = 1 << outside[rs.randint(len(outside))]
    return status


def reference_fit(gains, n_fft, steps=20):
    """float64 restatement of the estimator on ``np.fft``: per input, the nu in [-0.5, 0.5)
    that maximises ``|sum_c x[c] exp(-2 pi i c nu)|^2`` near the transform's peak (Newton steps
    from the peak until they vanish), and the phasor and amplitude there. NaN channels are 0."""
    x = np.where(np.isfinite(gains.real) & np.isfinite(gains.imag), gains, 0).astype(np.complex128)
    channels, n_inputs = x.shape
    power = np.abs(np.fft.fft(x, n_fft, axis=0)) ** 2
    nu = np.argmax(power, axis=0) / n_fft
    c = np.arange(channels)[:, np.newaxis]
    for _ in range(steps):
        e = x * np.exp(-2j * np.pi * c * nu)
        d0, d1, d2 = e.sum(axis=0), (c * e).sum(axis=0), (c * c * e).sum(axis=0)
        num = d1.imag * d0.real - d1.real * d0.imag
        den = 2 * np.pi * (np.abs(d1) ** 2 - (d2 * np.conj(d0)).real)
        nu = nu - num / den
    d0 = (x * np.exp(-2j * np.pi * c * nu)).sum(axis=0)
    kept = np.count_nonzero(x, axis=0)
    return nu - np.rint(nu), d0 / np.abs(d0), np.abs(d0) / kept


def assert_same(want, got, what=""):
    """Same dtype, shape and bit patterns; the one exception is a float (or a part of a
    complex number) that is NaN in `want`, which has to be a NaN in `got`."""
    assert want.dtype == got.dtype and want.shape == got.shape, what
    want, got = np.ascontiguousarray(want), np.ascontiguousarray(got)
    if want.dtype == np.uint8:
        nan = np.zeros(want.shape, bool)
        words_want, words_got, parts_got = want, got, got
    else:
        part, word = (np.float64, np.uint64) if want.dtype == np.float64 else (f32, np.uint32)
        parts_want, parts_got = want.view(part), got.view(part)
        words_want, words_got = want.view(word), got.view(word)
        nan = np.isnan(parts_want)
    bad = np.where(nan, ~np.isnan(parts_got), words_want != words_got)
    assert not bad.any(), (
        f"{what}: {np.count_nonzero(bad)} of {bad.size} words differ, first at "
        f"{np.argwhere(bad)[0]}: want {words_want[bad][0]:#x}, got {words_got[bad][0]:#x}")  # fmt: skip
