"""Seeded input generators shared by the golden-vector script and the tests.

Each generator reproduces the set-up of one of the reference's own tests (same seed,
same order of RandomState calls), so that the inputs need not be stored:
``np.random.RandomState`` legacy streams are frozen by NumPy's compatibility policy.
"""

import os

import numpy as np

BACKGROUND_COLS = [0, 1, 17, 99, 100, 312]
CFG1_COLS = [0, 1, 2, 3, 511, 1024, 2047]


def complex_normal(rs, size):
    """Circularly symmetric Gaussian, as reference test/__init__.py:31-42."""
    return rs.normal(0.0, 1.0, size) + 1j * rs.normal(0.0, 1.0, size)


def abs_probe():
    """complex64 probe values for numpy's abs: wide dynamic range plus specials."""
    rs = np.random.RandomState(5)
    n = 4096
    re = rs.standard_normal(n) * np.exp(rs.uniform(-20, 20, n))
    im = rs.standard_normal(n) * np.exp(rs.uniform(-20, 20, n))
    z = (re + 1j * im).astype(np.complex64)
    specials = np.array(
        [
            0, 1, 1j, -1, -1j, complex(-0.0, -0.0), complex(3, 4), complex(1e-45, 1e-45),
            complex(1e-45, 0), complex(3e38, 3e38), complex(3e38, 1e38), complex(1e-30, 1e-38),
            complex(np.inf, 1), complex(1, -np.inf), complex(np.inf, np.inf),
            complex(1e-20, 1e20), complex(1.1754944e-38, 1.1754944e-38),
        ],
        dtype=np.complex64,
    )  # fmt: skip
    return np.concatenate([z, specials])


def background_case():
    """reference test/rfi/test_background.py:33-45 (417x313, 10 % flags, block of 4s)."""
    shape = (417, 313)
    rs = np.random.RandomState(seed=1)
    vis_big = complex_normal(rs, size=shape).astype(np.complex64)
    flags_big = (rs.random_sample(shape) < 0.1).astype(np.uint8)
    flags_big[100:110, 0:100] = 4
    return vis_big, flags_big


def noise_case():
    """reference test/rfi/test_noise_est.py:39-43 (117x273 standard normal float32)."""
    rs = np.random.RandomState(seed=1)
    return rs.standard_normal((117, 273)).astype(np.float32)


def threshold_case():
    """reference test/rfi/test_threshold.py:32-41 (117x273, 25 % spikes of +200)."""
    shape = (117, 273)
    rs = np.random.RandomState(seed=1)
    spikes = rs.random_sample(shape) < 0.25
    deviations = rs.standard_normal(shape).astype(np.float32) * 10.0
    deviations[spikes] += 200.0
    return deviations, spikes


def flagger_case():
    """reference test/rfi/test_flagger.py:36-52 (117x131, 1/16 RFI, 1/16 input flags = 2)."""
    shape = (117, 131)
    rs = np.random.RandomState(seed=1)
    vis = complex_normal(rs, size=shape)
    spikes = rs.random_sample(shape) < 1.0 / 16.0
    spikes = spikes.astype(np.uint8)
    rfi_amp = rs.random_sample(shape) * 20.0 + 50.0
    rfi_phase = rs.random_sample(shape) * (2j * np.pi)
    rfi = rfi_amp * np.exp(rfi_phase)
    vis += spikes * rfi
    vis = vis.astype(np.complex64)
    input_flags = (rs.random_sample(shape) < 1.0 / 16.0).astype(np.uint8) * 2
    return vis, spikes, input_flags


def generate_data(channels, baselines, seed=1):
    """reference scripts/rfiflagtest.py:35-44."""
    rs = np.random.RandomState(seed=seed)
    out = np.empty((channels, baselines), np.complex64)
    for i in range(channels):
        real = rs.standard_normal(size=baselines).astype(np.float32)
        imag = rs.standard_normal(size=baselines).astype(np.float32)
        out[i] = real + 1j * imag
    return out


def add_rfi(vis, seed=3, fraction=1.0 / 16.0):
    """Spikes as in test/rfi/test_flagger.py:42-50, row by row to bound memory."""
    rs = np.random.RandomState(seed=seed)
    out = np.array(vis, dtype=np.complex64, copy=True)
    for i in range(vis.shape[0]):
        s = rs.random_sample(vis.shape[1]) < fraction
        amp = rs.random_sample(vis.shape[1]) * 20.0 + 50.0
        phase = rs.random_sample(vis.shape[1]) * (2j * np.pi)
        out[i] = (out[i].astype(np.complex128) + s * (amp * np.exp(phase))).astype(np.complex64)
    return out


def config1():
    """BASELINE.json config 1: generate_data(1024, 2048)."""
    return generate_data(1024, 2048)


def config1_rfi():
    """Config 1 with injected RFI so that 'flags bit-identical' is not vacuous."""
    return add_rfi(config1())


def channel_mask(channels, seed=2, fraction=1.0 / 16.0):
    """Per-channel input-flag mask of SURVEY 8(d) / config 5."""
    return (np.random.RandomState(seed).random_sample(channels) < fraction).astype(np.uint8)


def add_rfi_sparse(vis, seed=3, fraction=1.0 / 16.0, block=256):
    """Same kind of interference as :func:`add_rfi` (amplitude U(50, 70), random phase on
    a random `fraction` of the samples) for arrays of 10^8 samples: amplitudes and
    phases are drawn for the hit samples only, in blocks of rows, in place of three
    full-size float64 draws. Modifies and returns `vis` (complex64)."""
    rs = np.random.RandomState(seed=seed)
    for r0 in range(0, vis.shape[0], block):
        part = vis[r0 : r0 + block]
        hit = rs.random_sample(part.shape) < fraction
        n = int(np.count_nonzero(hit))
        amp = rs.random_sample(n) * 20.0 + 50.0
        phase = rs.random_sample(n) * (2.0 * np.pi)
        part[hit] += (amp * np.exp(1j * phase)).astype(np.complex64)
    return vis


def threshold_wide_case(seed=11):
    """Deviations for SumThreshold with 6 and 8 windows: 273 channels x 117 baselines of
    unit noise (float32) with runs of 3..40 channels raised by 2.5..6 (broad, weak
    interference that only the wide windows can find) and a few strong spikes; noise
    estimates near 1. Returns (deviations [C][B] float32, noise [B] float32)."""
    rs = np.random.RandomState(seed)
    channels, baselines = 273, 117
    dev = rs.standard_normal((channels, baselines)).astype(np.float32)
    for b in range(baselines):
        for _ in range(3):
            start = rs.randint(0, channels - 40)
            length = rs.randint(3, 41)
            dev[start : start + length, b] += np.float32(2.5 + 3.5 * rs.random_sample())
        dev[rs.randint(0, channels, 2), b] += 40.0
    noise = (0.9 + 0.2 * rs.random_sample(baselines)).astype(np.float32)
    return dev, noise


def denormal_case(channels=4096):
    """Amplitudes that are small multiples of 2^-149 (float32 subnormals), 8 baselines: a
    constant level of 20 units with two isolated spikes, and at one band edge a pattern under
    which an even-count window yields a deviation of exactly +-2^-150 -- not zero, but zero
    once rounded to float32 -- whose being counted among the non-zero deviations changes the
    MAD (1 or 2 units of noise with it, 2 or 3 without: patterns found by search). Baselines
    0-3 carry the pattern at the lower edge, 4-7 mirrored at the upper one.
    Returns float32 [channels][8]."""
    patterns = [[21, 18, 19, 19, 19, 18, 20, 22, 21, 21], [22, 22, 21, 22, 22, 22, 18, 22, 21, 20],
                [20, 20, 21, 20, 21, 22, 22, 20, 19, 20], [19, 19, 18, 18, 20, 22, 21, 21, 20, 19]]
    units = np.full((channels, 8), 20.0)
    for b in range(8):
        edge = np.array(patterns[b % 4], dtype=np.float64)
        if b < 4:
            units[:10, b] = edge
            units[100, b], units[200, b] = 29, 23
        else:
            units[-10:, b] = edge[::-1]
            units[channels - 101, b], units[channels - 201, b] = 29, 23
    return (units * 2.0 ** -149).astype(np.float32)


# Non-finite amplitudes (tests/golden/make_golden_nonfinite.py). Channel numbers of the
# planted samples, per baseline of nonfinite_case(); golden slices are taken around them.
NONFINITE_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                "rfi_host_nonfinite_golden.npz")
NONFINITE_WIDTHS = (5, 13, 31, 63, 255)
NONFINITE_MAD_CHANNELS = (4096, 4097, 20000, 20001)
NONFINITE_CHANNELS = 4096
NONFINITE_PLANTED = {
    1: [1000, 1500, 2000, 2001],
    2: list(range(500, 540)),
    3: [800, 1200, 1600],
    4: [0, NONFINITE_CHANNELS - 1],
    5: [63, 64, 127, 128],
    8: [700, 701, 1300, 2500],
    9: [2222],
    11: list(range(3000, 3010)) + list(range(3500, 3800)),
}


NONFINITE_AMP_PLANTED = {0: [100, 400], 1: list(range(200, 220)) + [600, 601, 602],
                         2: [300, 301, 302, 700, 701], 3: list(range(400, 700))}


def nonfinite_rows(planted=None, halo=2, limit=None):
    """Sorted channel numbers within `halo` of a planted sample (runs: their two ends)."""
    rows = set()
    for chans in (planted or NONFINITE_PLANTED).values():
        chans = sorted(chans)
        ends = [c for i, c in enumerate(chans)
                if i in (0, len(chans) - 1) or chans[i - 1] != c - 1 or chans[i + 1] != c + 1]
        for c in ends:
            rows.update(range(c - halo, c + halo + 1))
    n = limit or NONFINITE_CHANNELS
    return sorted(r for r in rows if 0 <= r < n)


def nonfinite_case(channels=NONFINITE_CHANNELS, seed=21):
    """complex64 [channels][12] of unit noise with one kind of non-finite input per baseline:
    0 clean control; 1 isolated inf+0j, 0+inf*j, and inf+nan*j next to a NaN sample; 2 a run
    of 40 samples of 3e38+3e38j (finite components, |z| overflows to inf); 3 the |z| overflow
    boundary, 2.4e38+0j and 1.7e38+1.7e38j (finite) and 2.41e38+2.41e38j (inf); 4 inf at the
    band edges; 5 inf on both sides of the lane boundaries 63/64 and 127/128; 6 all inf;
    7 inf on every other channel; 8 infs that the input flags mask; 9 interference plus one
    inf; 10 clean; 11 a run of 10 infs and one of 300 (longer than any window).
    Returns (vis, input_flags [channels][12] uint8): 1/16 of the samples flagged with 2, and
    every inf of baseline 8 with 1."""
    rs = np.random.RandomState(seed)
    shape = (channels, 12)
    vis = complex_normal(rs, shape).astype(np.complex64)
    inf = np.float32(np.inf)
    vis[1000, 1] = complex(inf, 0)
    vis[1500, 1] = complex(0, inf)
    vis[2000, 1] = complex(inf, np.nan)
    vis[2001, 1] = complex(np.nan, 0)
    vis[500:540, 2] = complex(3e38, 3e38)
    vis[800, 3] = complex(2.4e38, 0)
    vis[1200, 3] = complex(1.7e38, 1.7e38)
    vis[1600, 3] = complex(2.41e38, 2.41e38)
    vis[[0, channels - 1], 4] = inf
    vis[[63, 64, 127, 128], 5] = inf
    vis[:, 6] = inf
    vis[::2, 7] = inf
    vis[[700, 701, 1300, 2500], 8] = inf
    spikes = rs.random_sample(channels) < 1.0 / 16.0
    rfi = (rs.random_sample(channels) * 20.0 + 50.0) * np.exp(rs.random_sample(channels) * 2j * np.pi)
    vis[:, 9] += (spikes * rfi).astype(np.complex64)
    vis[2222, 9] = inf
    vis[3000:3010, 11] = inf
    vis[3500:3800, 11] = inf
    flags = (rs.random_sample(shape) < 1.0 / 16.0).astype(np.uint8) * 2
    flags[[700, 701, 1300, 2500], 8] = 1
    return vis, flags


def nonfinite_amp_case(channels=1024, seed=22):
    """float32 amplitudes [channels][5] (``amplitudes=True`` input, which may be negative):
    0 isolated +inf and -inf; 1 runs of -inf (20 and 3); 2 negative finite amplitudes next
    to +-inf; 3 a run of 300 +inf (longer than the widest window); 4 clean, with negatives.
    Returns (amp, input_flags [channels][5] uint8)."""
    rs = np.random.RandomState(seed)
    amp = (rs.standard_normal((channels, 5)) + 3.0).astype(np.float32)
    amp[100, 0], amp[400, 0] = np.inf, -np.inf
    amp[200:220, 1] = -np.inf
    amp[600:603, 1] = -np.inf
    amp[300, 2], amp[301, 2], amp[302, 2] = -5.0, np.inf, -1e3
    amp[700, 2], amp[701, 2] = -np.inf, -2.0
    amp[400:700, 3] = np.inf
    amp[::37, 4] *= -1.0
    flags = (rs.random_sample(amp.shape) < 1.0 / 16.0).astype(np.uint8) * 2
    return amp, flags


def nonfinite_amp_nan_case(channels=1024, seed=22):
    """nonfinite_amp_case with NaN amplitudes in place of and next to the +-inf of columns
    0-2 (the background leaves a NaN out of every window, and its own deviation is 0):
    0 NaN in place of the +inf and on either side of the -inf; 1 NaN at both ends of and
    inside the long run of -inf, in the middle of the short one and behind it; 2 NaN in place
    of the +inf between the negative amplitudes and in front of the -inf. Columns 3 and 4 and
    the input flags are nonfinite_amp_case's."""
    amp, flags = nonfinite_amp_case(channels, seed)
    amp[100, 0] = np.nan
    amp[[399, 401], 0] = np.nan
    amp[[199, 200, 210, 219, 220], 1] = np.nan
    amp[[601, 603], 1] = np.nan
    amp[301, 2] = np.nan
    amp[699, 2] = np.nan
    return amp, flags


def nonfinite_mad_case(channels, seed=23):
    """float32 deviations [channels][6] for the MAD noise estimate: 0 a few +-inf among unit
    noise; 1 more than half of them inf; 2 exactly half inf (the even-count midpoint is
    (x + inf) / 2); 3 an odd count whose median |d| lies in (FLT_MAX/2, FLT_MAX]; 4 an even
    count whose float32 midpoint sum overflows; 5 a quarter of the samples zero, +-inf mixed."""
    rs = np.random.RandomState(seed)
    dev = rs.standard_normal((channels, 6)).astype(np.float32)
    idx = rs.permutation(channels)
    dev[idx[:3], 0] = np.inf
    dev[idx[3:5], 0] = -np.inf
    dev[idx[: channels // 2 + 7], 1] = np.where(rs.random_sample(channels // 2 + 7) < 0.5, np.inf, -np.inf)
    even = channels - (channels & 1)
    dev[even:, 2] = 0.0
    dev[idx[idx < even][: even // 2], 2] = -np.inf
    big = rs.uniform(2.0e38, 3.2e38, channels).astype(np.float32) * np.where(rs.random_sample(channels) < 0.5, 1, -1).astype(np.float32)
    odd = channels - 1 + (channels & 1)
    dev[:, 3] = big
    dev[odd:, 3] = 0.0
    dev[:, 4] = np.abs(big)
    dev[even:, 4] = 0.0
    dev[idx[: channels // 4], 5] = 0.0
    dev[idx[channels // 4 : channels // 4 + 9], 5] = np.inf
    dev[idx[channels // 4 + 9 : channels // 4 + 12], 5] = -np.inf
    return dev


def nonfinite_threshold_case(channels=256, seed=24):
    """float32 deviations [channels][8] and noise [8] for the thresholds: 0 control with
    spikes; 1 one +inf; 2 one -inf next to a strong spike; 3 +inf and -inf two channels
    apart (inside one window of 4); 4 +inf next to -inf; 5 noise +inf; 6 noise NaN; 7 a run of
    6 infs."""
    rs = np.random.RandomState(seed)
    dev = rs.standard_normal((channels, 8)).astype(np.float32)
    dev[rs.randint(0, channels, (6, 8)), np.arange(8)] += 40.0
    dev[50, 1] = np.inf
    dev[60, 2], dev[61, 2] = -np.inf, 30.0
    dev[100, 3], dev[102, 3] = np.inf, -np.inf
    dev[130, 4], dev[131, 4] = np.inf, -np.inf
    dev[140, 5] = np.inf
    dev[150, 6] = np.inf
    dev[200:206, 7] = np.inf
    noise = (0.9 + 0.2 * rs.random_sample(8)).astype(np.float32)
    noise[5] = np.inf
    noise[6] = np.nan
    return dev, noise


def nonfinite_golden():
    return np.load(NONFINITE_GOLDEN, allow_pickle=False)


def nonfinite_input(tag):
    """(input, input flags, amplitudes, golden rows, channel-mode flag column) of a case."""
    if tag == "cplx":
        vis, flags = nonfinite_case()
        return vis, flags, False, nonfinite_rows(), 8
    amp, flags = nonfinite_amp_case()
    return amp, flags, True, nonfinite_rows(NONFINITE_AMP_PLANTED, limit=amp.shape[0]), 3
