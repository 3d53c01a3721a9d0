"""NaN deviations for the stand-alone noise estimate and the baseline-major thresholds.

By the definition (``rfi.host.NoiseEstMADHost`` takes ``mag > 0``, the reference
``abs_dev[abs_dev > 0]``, the C oracle ``if (a > 0)``) a NaN deviation takes no part in the
median, exactly like a zero; by ``rfi.host.ThresholdSumHost`` a window that holds a NaN never
fires and a NaN sample is never flagged. Inside the flagger the background stage turns NaN into
0, so only callers that bring their own deviations can reach these cases.

:func:`nan_mad_case` builds the columns for the noise estimate, one class of NaN placement per
column; :func:`kernel_rule_model` is the rule that a bit-pattern rank search has when it does
nothing about NaN (a NaN is a non-zero value above +inf), which no column with a NaN and a
finite noise may satisfy; :func:`nan_threshold_case` builds the columns for the thresholds.
tests/test_nan_deviations.py checks, from the data, that every class is what it claims to be.
"""

import os

import numpy as np

MAD_NORMAL = 1.4826

# The reference's own NoiseEstMADHost on nan_mad_case (tests/golden/make_golden_nan_deviations.py)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "rfi_host_nan_deviations_golden.npz")  # fmt: skip
GOLDEN_CHANNELS = (4096, 4097, 20000, 20001)

# Bit patterns of the single-NaN classes: quiet, quiet with the sign set, the smallest
# signalling NaN, the largest pattern of all (what csrc/noise.hip gives to channels that do
# not exist) and the same with the sign set.
NAN_PATTERNS = (0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0xFFFFFFFF)


# One length below, at and above every point where the launchers of csrc/noise.hip change path.
# ksp_madnz_t: the workgroup kernel with 1, 2 and 4 values per thread (up to 256, 512, 1024
# channels), the wavefront kernel (1025..4096), the workgroup kernel with 24, 32, 40 and 64 (up
# to 6144, 8192, 10240, 16384), madnz_long.h staged in LDS (up to 36864) and streamed.
# ksp_madnz: the strip kernel (up to 4096), then the re-reading kernel.
MAD_CHANNELS = (1, 2, 3, 256, 257, 512, 513, 1024, 1025, 4095, 4096, 4097, 6144, 6145, 8192, 8193,
                10240, 10241, 16384, 16385, 36864, 36865, 65537)  # fmt: skip
# a second, partial workgroup of the 64-baseline channel-major kernel, a ragged strip of 8 and a
# ragged group of 4 wavefront baselines
MAD_COLUMNS = 67


def nan_of(pattern):
    return np.array([pattern], np.uint32).view(np.float32)[0]


def _base(rs, n):
    """Unit noise; from 10 channels on a tenth of it exact zeros (shorter columns keep every
    value, so that the classes of 2 and 3 channels are not emptied by chance)."""
    col = rs.standard_normal(n).astype(np.float32)
    if n >= 10:
        col[rs.random_sample(n) < 0.1] = 0.0
    return col


def _distinct(rs, m):
    """`m` values of distinct magnitudes in [1, 2), random signs, shuffled."""
    mags = (1.0 + rs.permutation(m) / np.float64(max(m, 1))).astype(np.float32)
    return mags * np.where(rs.random_sample(m) < 0.5, -1, 1).astype(np.float32)


def _constructed(rs, n, parity, tie=False):
    """One NaN, as many zeros as it takes for the non-zero count without the NaN to have
    `parity` (so the count with the NaN has the other), distinct magnitudes otherwise; with
    `tie` the two middle magnitudes are equal and there are three NaN (with one, the upper
    median alone, which the other rule would give, is the same value)."""
    n_nan = 3 if tie else 1
    zeros = (n - n_nan - parity) % 2
    m = n - n_nan - zeros
    vals = _distinct(rs, m)
    if tie:
        order = np.argsort(np.abs(vals))
        vals[order[m // 2 - 1]] = -vals[order[m // 2]]  # same magnitude, other sign
    col = np.concatenate([vals, np.zeros(zeros, np.float32), np.full(n_nan, np.nan, np.float32)])
    return col[rs.permutation(n)].astype(np.float32)


def handover_positions(n):
    """Channel 0, the last channel and both sides of every multiple of 64 (which holds the
    multiples of 256) below `n`: where one lane's or one thread's run of channels ends and
    the next one's begins."""
    pos = {0, n - 1}
    for c in range(64, n, 64):
        pos.update((c - 1, c))
    return np.array(sorted(pos))


def _single(pattern):
    def build(rs, n):
        col = _base(rs, n)
        col[rs.randint(n)] = nan_of(pattern)
        return col

    return build


def _scattered(rs, n):
    col = _base(rs, n)
    col[rs.permutation(n)[: max(1, n // 10)]] = np.nan
    return col


def _majority(rs, n):
    col = _base(rs, n)
    col[rs.permutation(n)[: n // 2 + 1]] = np.nan
    return col


def _all_but_one(rs, n):
    col = np.full(n, np.nan, np.float32)
    col[rs.randint(n)] = 2.0
    return col


def _nan_and_zeros(rs, n):
    col = np.zeros(n, np.float32)
    col[rs.permutation(n)[: (n + 1) // 2]] = np.nan
    return col


def _mixed(rs, n):
    col = _base(rs, n)
    idx = rs.permutation(n)
    k = max(1, n // 16)
    col[idx[:k]] = np.nan
    col[idx[k : 2 * k]] = 0.0
    col[idx[2 * k : 3 * k]] = -0.0
    col[idx[3 * k : 4 * k]] = np.inf
    col[idx[4 * k : 5 * k]] = -np.inf
    return col


def _handovers(rs, n):
    col = _base(rs, n)
    col[handover_positions(n)] = np.nan
    return col


# (name, least number of channels at which the class can be built and still differs from the
# classes of fewer NaN, builder). The rule for leaving a class out is the middle entry alone.
CLASSES = (
    ("control", 1, lambda rs, n: _base(rs, n)),
    ("one_quiet", 2, _single(0x7FC00000)),
    ("pattern_7fc00000", 2, _single(NAN_PATTERNS[0])),
    ("pattern_ffc00000", 2, _single(NAN_PATTERNS[1])),
    ("pattern_7f800001", 2, _single(NAN_PATTERNS[2])),
    ("pattern_7fffffff", 2, _single(NAN_PATTERNS[3])),
    ("pattern_ffffffff", 2, _single(NAN_PATTERNS[4])),
    ("one_in_ten", 10, _scattered),
    ("majority", 3, _majority),
    ("all_but_one", 2, _all_but_one),
    ("all", 1, lambda rs, n: np.full(n, np.nan, np.float32)),
    ("nan_and_zeros", 2, _nan_and_zeros),
    ("mixed", 8, _mixed),
    # even count, the two middle values distinct: the upper median is the first sample of its
    # value, the `below == rank` branch of every kernel
    ("even_first", 3, lambda rs, n: _constructed(rs, n, 0)),
    ("odd", 2, lambda rs, n: _constructed(rs, n, 1)),
    # even count, the two middle values equal: the other side of that branch
    ("even_tie", 5, lambda rs, n: _constructed(rs, n, 0, tie=True)),
    ("handovers", 3, _handovers),
)


def classes_at(channels):
    """Names of the classes that `channels` channels allow, in column order."""
    return [name for name, least, _ in CLASSES if channels >= least]


def column_class(channels, b):
    names = classes_at(channels)
    return names[b % len(names)]


def nan_mad_case(channels, columns, seed=31):
    """float32 deviations [channels][columns]; column ``b`` has class
    ``classes_at(channels)[b % n_classes]`` and data of its own."""
    builders = {name: build for name, _, build in CLASSES}
    names = classes_at(channels)
    dev = np.empty((channels, columns), np.float32)
    for b in range(columns):
        rs = np.random.RandomState([seed, channels, b])
        col = builders[names[b % len(names)]](rs, channels)
        assert col.shape == (channels,) and col.dtype == np.float32
        dev[:, b] = col
    return dev


def reference_rule(dev):
    """The reference's rule written out: ``median(a[a > 0]) * 1.4826`` per column, the median in
    float32, NaN where nothing is left; float32."""
    out = np.empty(dev.shape[1], np.float64)
    for b in range(dev.shape[1]):
        a = np.abs(dev[:, b])
        a = a[a > 0]
        with np.errstate(all="ignore"):
            out[b] = np.median(a) if a.size else np.nan
    return (out * MAD_NORMAL).astype(np.float32)


def kernel_rule_model(dev):
    """What a rank search on the 31-bit magnitude patterns gives when a NaN is a non-zero value
    above +inf: zeros are the all-clear patterns, the target rank is ``(n + zeros) // 2`` among
    all ``n`` patterns, an even ``n + zeros`` averages it with the rank below in float32."""
    n = dev.shape[0]
    out = np.empty(dev.shape[1], np.float64)
    for b in range(dev.shape[1]):
        keys = np.sort(np.ascontiguousarray(dev[:, b]).view(np.uint32) & np.uint32(0x7FFFFFFF))
        zeros = int(np.count_nonzero(keys == 0))
        if zeros == n:
            out[b] = np.nan
            continue
        rank2 = n + zeros
        vals = keys.view(np.float32)
        med = vals[rank2 // 2]
        if rank2 % 2 == 0:
            with np.errstate(all="ignore"):
                med = (med + vals[rank2 // 2 - 1]) * np.float32(0.5)
        out[b] = med
    return (out * MAD_NORMAL).astype(np.float32)


# ------------------------------------------------------------------------------ thresholds
THRESHOLD_N_SIGMA = 11.0
THRESHOLD_FALLOFF = 1.2
THRESHOLD_CHANNELS = (257, 2100)


def sum_edge(n_windows):
    """The halo of a chunk of threshold_sum_kernel (csrc/threshold.hip, ksp_threshold_sum)."""
    return (1 << n_windows) - n_windows - 1


def chunk_positions(channels):
    """Channels next to the boundaries of threshold_sum_kernel that do not fall on a multiple
    of 8, as read from csrc/threshold.hip. Only ``vt = 8`` cuts 2100 channels in two chunks
    (``tot = 2048``); with ``n`` windows ``edge = 2^n - n - 1`` and ``core = tot - 2 * edge``:

    * chunk 1's core starts at ``core`` (chunk 0 writes flags up to ``core - 1``),
    * chunk 1's halo starts at ``core - edge``, chunk 0's ends at ``core + edge``,
    * thread ``t`` of chunk 0 owns local positions ``[8 t, 8 t + 8)`` = channels from
      ``8 t - edge``, thread ``t`` of chunk 1 those from ``core - edge + 8 t``.

    Returns the sorted channels ``b - 1, b`` for each such boundary ``b`` inside the band."""
    pos = set()
    if channels <= 2048:  # one chunk whatever vt is: no halo, hand-overs on multiples of 8
        return np.array([], np.int64)
    for n_windows in range(1, 9):
        edge = sum_edge(n_windows)
        core = 2048 - 2 * edge
        bounds = [core, core - edge, core + edge]
        bounds += [8 * t - edge for t in (1, 2, 100, 255)]  # thread hand-overs of chunk 0
        bounds += [core - edge + 8 * t for t in (1, 2, 30)]  # ... and of chunk 1
        for b in bounds:
            if 1 <= b < channels:
                pos.update((b - 1, b))
    return np.array(sorted(pos), np.int64)


# The runs of column 3..5: (k, first channel); 2^k samples that fire only as a window of 2^k.
THRESHOLD_RUNS = {3: ((1, 20), (2, 40), (3, 60), (4, 90), (5, 130)), 4: ((6, 100),), 5: ((7, 64),)}
# The spikes of column 2 with a NaN on the left, on the right and on both sides
THRESHOLD_SPIKES = ((50, (49,)), (120, (121,)), (200, (199, 201)))


def nan_threshold_case(channels, seed=32, with_nan=True):
    """float32 deviations [channels][12] and noise [12] for the baseline-major thresholds;
    `with_nan` False gives the control, the same without any NaN (the NaN samples keep the
    value they had before). Columns:

    0 control: unit noise with strong spikes, no NaN;
    1 the same with isolated NaN;
    2 spikes that fire alone, a NaN on their left, on their right and on both sides;
    3 runs of 2, 4, 8, 16 and 32 samples just above their window's threshold, a NaN in the
      middle of each; 4 the same for 64 and 5 for 128 samples;
    6 a whole row of NaN;
    7 a NaN at channel 0 and at the last channel, a spike next to each;
    8 a NaN on both sides of the channels 8, 16, 32, 64, 128 and 256: the hand-over between two
      threads' ``VT`` = 8, 16 or 32 channels while one chunk holds the band, spikes around them;
    9 a NaN on both sides of every multiple of 8, a spike two channels behind every fourth;
    10 a NaN on both sides of every boundary of :func:`chunk_positions` (none at 257
      channels: the column is then a second control), spikes around them;
    11 column 10's NaN inside a long stretch that every window flags.
    """
    rs = np.random.RandomState([seed, channels])
    dev = rs.standard_normal((channels, 12)).astype(np.float32)
    noise = (0.9 + 0.2 * rs.random_sample(12)).astype(np.float32)
    nan = np.zeros(dev.shape, bool)
    thr1 = np.float32(THRESHOLD_N_SIGMA) * noise

    for b in (0, 1):
        dev[rs.randint(0, channels, 6), b] += 40.0
    iso = rs.permutation(channels)[:5]
    nan[iso, 1] = True
    for spike, nans in THRESHOLD_SPIKES:
        dev[spike, 2] = 40.0
        nan[list(nans), 2] = True
    for b, runs in THRESHOLD_RUNS.items():
        dev[:, b] *= np.float32(0.05)  # a quiet column: the runs alone decide
        for k, start in runs:
            level = np.float32(thr1[b] * np.float32(THRESHOLD_FALLOFF**-k) * np.float32(1.1))
            dev[start : start + 2**k, b] = level
            nan[start + 2**k // 2, b] = True
    nan[:, 6] = True
    dev[[1, channels - 2], 7] = 40.0
    nan[[0, channels - 1], 7] = True
    for c in (8, 16, 32, 64, 128, 256):
        dev[c - 2, 8] = 40.0
        if c + 1 < channels:
            dev[c + 1, 8] = 40.0
        nan[[c - 1, c], 8] = True
    for c in range(8, channels, 8):
        nan[[c - 1, c], 9] = True
        if c % 32 == 0 and c + 2 < channels:
            dev[c + 2, 9] = 40.0
    pos = chunk_positions(channels)
    nan[pos, 10] = True
    for c in pos[::2]:
        if c >= 1 and not nan[c - 1, 10]:
            dev[c - 1, 10] = 40.0
    for c in pos[1::2]:
        if c + 1 < channels and not nan[c + 1, 10]:
            dev[c + 1, 10] = 40.0
    if pos.size:
        dev[1200:, 11] = 500.0
        nan[pos[pos >= 1200], 11] = True
    if with_nan:
        dev[nan] = np.nan
    return dev, noise
