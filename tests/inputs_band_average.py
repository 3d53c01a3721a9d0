"""Inputs of the band-average tests (tests/test_band_average.py checks the host class with
them, tests/test_gpu_band_average.py runs them on the device), and the independent statement
of ``rfi.host.BandAverageHost`` that the CPU test compares with: a triple loop of
``np.float32`` scalars."""

import numpy as np

f32 = np.float32
c64 = np.complex64
TINY = f32(2.0**-149)  # the smallest denormal
HUGE = f32(2.0**127)
BLOCK = 128
NAMES = ("mean", "mean_amplitude", "weight_sums", "counts", "series_flags")
MASK = 0x01
OTHER_BIT = 0x20


def make_data(seed, channels, baselines, cancelling=True):
    """complex64 (channels, baselines): standard normal parts. With `cancelling`, the last
    baseline holds values near +-2^20 in turn, whose sums lose everything to the order in which
    they are taken."""
    rs = np.random.RandomState(seed)
    shape = (channels, baselines)
    data = (rs.standard_normal(shape) + 1j * rs.standard_normal(shape)).astype(c64)
    if cancelling:
        sign = np.where(np.arange(channels) % 2 == 0, 1.0, -1.0)
        big = sign * 2.0**20 * (1 + rs.random_sample(channels) * 2.0**-6)
        data[:, -1] = (big + 1j * big[::-1]).astype(c64) + data[:, -1]
    return data


def make_weights(seed, n_series, channels, zero=0.3):
    """float32 (n_series, channels): non-dyadic weights in (0.1, 1.1), a fraction `zero` of them
    zero."""
    rs = np.random.RandomState(seed)
    weights = (0.1 + rs.random_sample((n_series, channels))).astype(f32)
    weights[rs.random_sample(weights.shape) < zero] = 0
    return weights


def make_flags(seed, shape, fraction=0.3):
    """uint8 flags: MASK on about `fraction` of the samples, OTHER_BIT on about a tenth,
    independently."""
    rs = np.random.RandomState(seed)
    flags = np.where(rs.random_sample(shape) < fraction, MASK, 0).astype(np.uint8)
    flags |= np.where(rs.random_sample(shape) < 0.1, OTHER_BIT, 0).astype(np.uint8)
    return flags


def loop_reference(data, channel_weights, flags, mask):
    """The definition, one float32 scalar operation at a time."""
    channels, baselines = data.shape
    n_series = channel_weights.shape[0]
    zero = f32(0)
    mean = np.zeros((n_series, baselines), c64)
    mean_amplitude = np.zeros((n_series, baselines), f32)
    weight_sums = np.zeros((n_series, baselines), f32)
    counts = np.zeros((n_series, baselines), np.uint32)
    series_flags = None if flags is None else np.zeros((n_series, baselines), np.uint8)
    with np.errstate(all="ignore"):
        amplitude = np.abs(data)
        for k in range(n_series):
            for b in range(baselines):
                total = [zero, zero, zero, zero]
                for start in range(0, channels, BLOCK):
                    partial = [zero, zero, zero, zero]
                    for c in range(start, min(start + BLOCK, channels)):
                        w = channel_weights[k, c]
                        if not w > 0:
                            continue
                        if flags is not None:
                            series_flags[k, b] |= flags[c, b]
                        re, im = data[c, b].real, data[c, b].imag
                        if np.isnan(re) or np.isnan(im):
                            continue
                        if flags is not None and flags[c, b] & mask:
                            continue
                        terms = (f32(w * re), f32(w * im), f32(w * amplitude[c, b]), w)
                        partial = [f32(p + t) for p, t in zip(partial, terms)]
                        counts[k, b] += 1
                    total = [f32(s + p) for s, p in zip(total, partial)]
                weight_sums[k, b] = total[3]
                if total[3] > 0:
                    mean[k, b] = complex(f32(total[0] / total[3]), f32(total[1] / total[3]))
                    mean_amplitude[k, b] = f32(total[2] / total[3])
    return mean, mean_amplitude, weight_sums, counts, series_flags


def special_case():
    """(data, channel_weights, flags, mask) with every special value of the definition, 300
    channels (three blocks) by 12 baselines, four series:

    series 0: random weights; series 1: all zero, negative or NaN; series 2: ones; series 3:
    2^-140 (denormal products and sums).
    baseline 0: ordinary; 1: a NaN real part and a NaN imaginary part among ordinary samples;
    2: +inf real parts, kept; 3: everything flagged under the mask; 4: all NaN; 5: flagged
    samples only in channels whose weight in series 0 is 0; 6: denormal data; 7: zeros and
    negative zeros; 8..11: ordinary with random flags."""
    channels, baselines = 300, 12
    rs = np.random.RandomState(77)
    data = make_data(78, channels, baselines, cancelling=False)
    weights = make_weights(79, 4, channels)
    weights[1] = np.array([0, -1, np.nan, -0.0, -np.inf], f32)[rs.randint(5, size=channels)]
    weights[2] = 1
    weights[3] = f32(2.0**-140)
    flags = np.zeros((channels, baselines), np.uint8)
    flags[:, 8:] = make_flags(80, (channels, 4))
    data[[3, 130], 1] = complex(np.nan, 1)
    data[[4, 299], 1] = complex(1, np.nan)
    data[[0, 127, 128, 200], 2] = complex(np.inf, -2)
    flags[:, 3] = MASK | np.where(np.arange(channels) % 3 == 0, OTHER_BIT, 0).astype(np.uint8)
    data[:, 4] = complex(np.nan, np.nan)
    data[::2, 4] = complex(np.nan, 3)
    flags[:, 4] = np.where(np.arange(channels) % 5 == 0, 0x80, 0).astype(np.uint8)
    out_of_series0 = weights[0] == 0
    assert 50 < out_of_series0.sum() < 150
    flags[out_of_series0, 5] = MASK | 0x40
    data[:, 6] = (data[:, 6] * f32(2.0**-135)).astype(c64)
    data[:, 7] = np.array([0, -0.0, complex(0, -0.0), complex(-0.0, -0.0)], c64)[
        rs.randint(4, size=channels)]  # fmt: skip
    return data, weights, flags, MASK
