"""Seeded inputs for the tests of ``rfi.host.PredictHost`` and of the device operation
(tests/test_predict.py, tests/test_gpu_predict.py): frequencies, delays and fluxes of several
kinds, the samples to divide, a longdouble reference and the comparison both use."""

import numpy as np

from tests.inputs_apply_gains import assert_same, make_flags, make_vis, make_weights  # noqa: F401

f32 = np.float32

#: kinds of :func:`make_model`
PATTERNS = ("random", "large", "exact", "huge", "nonfinite", "flux", "cancel")
#: what the ``flux`` pattern sprinkles over the ordinary fluxes, about 8 % of the elements each
SPECIAL_FLUX = (0.0, -0.0, 1e-30, -1e-30, 3e38, -3e38, 2.0**-149)


def make_flux(rs, channels, n_sources):
    """float32 (channels, n_sources): normal deviates times 2^U(-3, 3), both signs."""
    shape = (channels, n_sources)
    return (rs.standard_normal(shape) * np.exp2(rs.uniform(-3, 3, shape))).astype(f32)


def make_model(seed, channels, baselines, n_sources, pattern="random"):
    """dict of freqs (channels,) float64, delays (n_sources, baselines) float64 and flux
    (channels, n_sources) float32.

    ``random``: a band around 1 GHz and delays of up to a microsecond (a thousand turns);
    ``large``: frequencies up to 2^30 Hz and delays up to 2^-10 s: up to 2^20 turns;
    ``exact``: frequencies 1, 2, 4, 8 and delays that are whole eighths (and -0), so every x
    is exact and r is 0, +-1/8, +-1/4, +-3/8 or +-1/2: both rint()s meet their ties;
    ``huge``: |x| of 2^51 (with halves: ties of the first rint at the largest magnitude that
    has any) up to 2^60 and more, where r = 0;
    ``nonfinite``: ``random`` with NaN and +-inf in about 3 % of freqs, delays and flux each;
    ``flux``: ``random`` with each of SPECIAL_FLUX in about 8 % of the fluxes (a model of
    zero, one whose d underflows, one whose d overflows), and the whole first channel zero;
    ``cancel``: the sources come in pairs with the same delays and opposite fluxes (an odd one
    out has no flux), so every model is exactly zero."""
    assert pattern in PATTERNS
    rs = np.random.RandomState(seed)
    freqs = np.sort(rs.uniform(0.85e9, 1.71e9, channels))
    delays = rs.uniform(-1e-6, 1e-6, (n_sources, baselines))
    flux = make_flux(rs, channels, n_sources)
    if pattern == "large":
        freqs = np.sort(rs.uniform(0.5, 1.0, channels)) * 2.0**30
        delays = rs.uniform(-1.0, 1.0, (n_sources, baselines)) * 2.0**-10
    elif pattern == "exact":
        freqs = np.exp2(np.arange(channels) % 4).astype(np.float64)
        delays = rs.randint(-40, 41, (n_sources, baselines)) / 8.0
        delays[rs.random_sample(delays.shape) < 0.05] = -0.0
    elif pattern == "huge":
        freqs = np.exp2(40 + np.arange(channels) % 3).astype(np.float64)
        mantissa = rs.randint(-(2**20), 2**20, (n_sources, baselines)).astype(np.float64)
        delays = mantissa * np.exp2(rs.randint(-10, 12, (n_sources, baselines)))
        # x = 2^51 + k / 2 for the first channel: the last binade with a half in it
        ties = rs.random_sample(delays.shape) < 0.3
        halves = (2.0**52 + rs.randint(0, 64, delays.shape)) * 2.0**-41
        delays = np.where(ties, np.where(rs.random_sample(delays.shape) < 0.5, halves, -halves),
                          delays)  # fmt: skip
    elif pattern == "nonfinite":
        for array in (freqs, delays, flux):
            kind = rs.random_sample(array.shape)
            for i, value in enumerate([np.nan, np.inf, -np.inf]):
                array[(kind >= 0.01 * i) & (kind < 0.01 * (i + 1))] = value
        if channels > 3:  # (whole rows, whatever the seed)
            freqs[1], freqs[channels // 2], freqs[-1] = np.nan, np.inf, -np.inf
        delays[0, baselines // 2] = np.nan
    elif pattern == "flux":
        kind = rs.random_sample(flux.shape)
        for i, value in enumerate(SPECIAL_FLUX):
            flux[(kind >= 0.08 * i) & (kind < 0.08 * (i + 1))] = value
        flux[0] = 0
        if channels > 1:
            flux[1] = f32(1e-30)
        if channels > 2:
            flux[2] = f32(3e38)
    elif pattern == "cancel":
        delays[1::2] = delays[0 : 2 * (n_sources // 2) : 2]
        flux[:, 1::2] = -flux[:, 0 : 2 * (n_sources // 2) : 2]
        if n_sources % 2:
            flux[:, -1] = 0
    return {"freqs": np.ascontiguousarray(freqs, np.float64),
            "delays": np.ascontiguousarray(delays, np.float64),
            "flux": np.ascontiguousarray(flux, f32)}  # fmt: skip


def make_case(seed, channels, baselines, n_sources, pattern="random", flag_value=64):
    """dict of freqs, delays, flux, vis, weights, flags for one shape."""
    case = make_model(seed, channels, baselines, n_sources, pattern)
    case["vis"] = make_vis(seed + 1, channels, baselines)
    case["weights"] = make_weights(seed + 2, channels, baselines)
    case["flags"] = make_flags(seed + 3, channels, baselines, flag_value)
    return case


def reference_model(freqs, delays, flux):
    """complex longdouble (channels, baselines): sum_s flux[c, s] exp(-2 pi i (x - rint(x)))
    with x = freqs[c] * delays[s, j] as float64 gives it; x - rint(x) is exact."""
    ld = np.longdouble
    two_pi = 8 * np.arctan(ld(1))
    total = np.zeros((len(freqs), delays.shape[1]), np.clongdouble)
    for s in range(delays.shape[0]):
        x = freqs[:, np.newaxis] * delays[s][np.newaxis, :]
        angle = two_pi * (x - np.rint(x)).astype(ld)
        amplitude = flux[:, s, np.newaxis].astype(ld)
        total += amplitude * np.cos(angle) - 1j * (amplitude * np.sin(angle))
    return total
