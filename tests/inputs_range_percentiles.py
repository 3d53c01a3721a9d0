"""Inputs of the range-percentile tests (tests/test_range_percentiles.py checks what they
contain, tests/test_gpu_range_percentiles.py runs them on the device), and the independent
statement of ``rfi.host.RangePercentilesHost`` that both compare with."""

import numpy as np

f32 = np.float32
c64 = np.complex64
TINY = f32(2.0**-149)  # the smallest denormal
HUGE = f32(2.0**127)
ROW_ORDER = [0, 100, 25, 75, 50]

# complex samples whose |z| is not an ordinary number, with what numpy.abs makes of them
COMPLEX_SPECIALS = [
    (complex(np.nan, 1), np.nan), (complex(1, np.nan), np.nan), (complex(np.inf, np.nan), np.inf),
    (complex(3e38, 3e38), np.inf), (0j, 0.0), (complex(float(TINY), 0), float(TINY)),
    (complex(0, 3 * float(TINY)), 3 * float(TINY)), (complex(np.inf, 1), np.inf),
]  # fmt: skip
FLOAT_SPECIALS = [np.nan, np.inf, 0.0, float(TINY), 2.0**-130, 1e-40]


def make_data(seed, channels, baselines, dtype, special=0.08, distinct=37):
    """(channels, baselines) of `dtype` (float32: non-negative amplitudes). Three samples in
    four come from `distinct` values (exact ties; complex ones also as their conjugates,
    negatives and with the parts swapped, which have the same amplitude), the rest are
    2^U(-20, 20); a fraction `special` is NaN, +inf, zero or denormal."""
    rs = np.random.RandomState(seed)
    shape = (channels, baselines)
    complex_ = np.dtype(dtype) == c64
    if complex_:
        pool = (rs.standard_normal(distinct) + 1j * rs.standard_normal(distinct)).astype(c64)
        pool *= np.exp2(rs.randint(-8, 9, distinct)).astype(f32)
        free = (rs.standard_normal(shape) + 1j * rs.standard_normal(shape)).astype(c64)
        free *= np.exp2(rs.uniform(-20, 20, shape)).astype(f32)
    else:
        pool = np.exp2(rs.uniform(-8, 8, distinct)).astype(f32)
        free = np.exp2(rs.uniform(-20, 20, shape)).astype(f32)
    data = pool[rs.randint(distinct, size=shape)]
    if complex_:
        variant = rs.randint(4, size=shape)
        data = np.where(variant == 1, np.conj(data), data)
        data = np.where(variant == 2, -data, data)
        data = np.where(variant == 3, data.imag + 1j * data.real, data).astype(c64)
    data = np.where(rs.random_sample(shape) < 0.25, free, data).astype(dtype)
    what = rs.random_sample(shape)
    specials = [z for z, _ in COMPLEX_SPECIALS] if complex_ else FLOAT_SPECIALS
    step = special / len(specials)
    for i, value in enumerate(specials):
        data[(what >= i * step) & (what < (i + 1) * step)] = value
    return data


def make_flags(seed, shape, fraction=0.25):
    """uint8 flags: bit 0x01 on about `fraction` of the samples, bits 0x08, 0x20 and 0x80 each
    on about a tenth, independently."""
    rs = np.random.RandomState(seed)
    flags = np.where(rs.random_sample(shape) < fraction, 0x01, 0).astype(np.uint8)
    for bit in (0x08, 0x20, 0x80):
        flags |= np.where(rs.random_sample(shape) < 0.1, bit, 0).astype(np.uint8)
    return flags


KEPT_COUNTS = ["0", "1", "2", "3", "4", "5", "8", "n-1", "n"]


def kept_count_case(seed, length, dtype, start=3, tail=2):
    """(data, flags, ranges, kept): one row per entry of KEPT_COUNTS with exactly that many
    samples of the one range (start, start + length) kept under mask 0x01; NaN-free data, so
    the flags alone decide. The columns around the range are unflagged."""
    rs = np.random.RandomState(seed)
    kept = [length - 1 if k == "n-1" else length if k == "n" else int(k) for k in KEPT_COUNTS]
    baselines = start + length + tail
    data = make_data(seed, len(kept), baselines, dtype, special=0.0)
    flags = make_flags(seed + 1, data.shape, 0.0) & np.uint8(0xFE)
    for row, n in enumerate(kept):
        flagged = rs.permutation(length)[: length - n] + start
        flags[row, flagged] |= 0x01
    return data, flags, [(start, start + length)], kept


# sixteen ranges on a row of 5000: overlapping, nested, repeated, out of order, empty ones
# first, in the middle and last, the whole row, a single column, odd starts
LAYOUT_BASELINES = 5000
LAYOUT_RANGES = [
    (7, 7), (0, 5000), (4999, 5000), (1, 64), (33, 1057), (100, 300), (100, 300), (2500, 2500),
    (4001, 4999), (3, 260), (301, 2349), (0, 1), (1235, 4996), (64, 128), (555, 4651),
    (5000, 5000),
]  # fmt: skip


def loop_reference(data, flags, ranges, mask):
    """The definition, one (channel, range) at a time, through numpy.percentile."""
    channels = data.shape[0]
    percentiles = np.zeros((len(ranges), 5, channels), f32)
    counts = np.zeros((len(ranges), channels), np.uint32)
    range_flags = None if flags is None else np.zeros((len(ranges), channels), np.uint8)
    with np.errstate(all="ignore"):
        amplitude = np.abs(data) if data.dtype == c64 else data
    for r, (start, stop) in enumerate(ranges):
        for c in range(channels):
            a = amplitude[c, start:stop]
            keep = ~np.isnan(a)
            if flags is not None:
                keep &= (flags[c, start:stop] & mask) == 0
                for value in flags[c, start:stop]:
                    range_flags[r, c] |= value
            k = a[keep]
            counts[r, c] = len(k)
            if len(k):
                with np.errstate(all="ignore"):
                    percentiles[r, :, c] = np.percentile(k, ROW_ORDER, method="lower")
    return percentiles, counts, range_flags
