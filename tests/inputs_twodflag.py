"""Seeded inputs of the 2-D SumThreshold flagger cases, shared by
``golden/make_golden_twodflag.py`` and the tests that check against its fixture."""

import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "rfi_twodflag_golden.npz")  # fmt: skip
#: the reference's stages, per baseline in call order, for STAGE_CASES
STAGES_GOLDEN = os.path.join(os.path.dirname(GOLDEN), "rfi_twodflag_stages_golden.npz")

#: 32 time windows, unsorted and with duplicates (the reference keeps both)
WINDOWS_TIME_32 = [3, 1, 2, 2, 5, 8, 1, 13, 4, 4, 6, 21, 7, 3, 9, 11, 2, 17, 10, 5, 16, 12, 1, 14,
                   15, 30, 8, 19, 24, 6, 27, 40]  # fmt: skip

#: name -> (shape (time, channels, baselines), kind, seed, constructor keywords)
CASES = {
    "default": ((48, 512, 3), "rfi", 1, {}),
    "chunks1": ((32, 96, 2), "rfi", 2, {"freq_chunks": 1}),
    "chunks_many": ((32, 24, 2), "rfi", 3, {"freq_chunks": 40}),
    "avg1_chunks7": ((24, 70, 2), "rfi", 4, {"freq_chunks": 7, "average_freq": 1}),
    "avg3": ((32, 100, 2), "rfi", 5, {"average_freq": 3}),
    "avg4": ((32, 128, 2), "rfi", 6, {"average_freq": 4}),
    "iter1": ((40, 96, 2), "rfi", 7, {"background_iterations": 1, "spike_width_time": 4.0}),
    "iter3": ((40, 96, 2), "rfi", 8, {"background_iterations": 3}),
    "windows": ((24, 50, 2), "rfi", 9, {"windows_time": [1, 2, 40], "windows_freq": [1, 3, 200]}),
    "preflagged": ((32, 96, 2), "preflagged", 10, {}),
    "nans": ((32, 96, 2), "nans", 11, {}),
    "all_flagged": ((16, 40, 2), "all_flagged", 12, {}),
    "amplitudes": ((32, 96, 2), "amplitudes", 13, {}),
    "n_time_1": ((1, 64, 2), "rfi", 14, {}),
    "odd": ((31, 77, 3), "rfi", 15, {"time_extend": 5, "freq_extend": 1, "freq_chunks": 3}),
    # every constructor parameter away from its default, and the data classes where
    # medians, sums and comparisons go wrong
    "nsigma_rho1": ((24, 64, 2), "rfi", 16, {"outlier_nsigma": 3.0, "rho": 1.0,
                                             "background_reject": 1.5}),
    "rho2": ((24, 64, 2), "rfi", 17, {"outlier_nsigma": 6.0, "rho": 2.0, "background_reject": 3.5,
                                      "windows_time": [1, 2], "windows_freq": [2, 1],
                                      "time_extend": 1, "freq_extend": 2}),
    "iter0": ((24, 64, 2), "rfi", 18, {"background_iterations": 0}),
    "wide_box": ((16, 96, 2), "rfi", 19, {"background_iterations": 2, "spike_width_time": 40.0,
                                          "spike_width_freq": 45.0, "freq_chunks": 4}),
    "spike_time0": ((24, 64, 2), "rfi", 20, {"spike_width_time": 0.0}),
    "spike_freq0": ((24, 64, 2), "rfi", 21, {"spike_width_freq": 0.0, "time_extend": 2,
                                             "freq_extend": 6}),
    "extend4_6": ((24, 64, 2), "rfi", 22, {"time_extend": 4, "freq_extend": 6,
                                           "flag_all_time_frac": 1.0, "flag_all_freq_frac": 1.0}),
    "frac0": ((16, 48, 2), "rfi", 23, {"flag_all_time_frac": 0.0, "flag_all_freq_frac": 0.0}),
    "frac_exact": ((16, 32, 1), "blocks", 24, {"windows_time": [1], "windows_freq": [1],
                                               "freq_chunks": 1,
                                               "time_extend": 1, "freq_extend": 1,
                                               "flag_all_time_frac": 0.125,
                                               "flag_all_freq_frac": 0.125}),
    "windows32": ((40, 72, 2), "rfi", 25, {"windows_time": WINDOWS_TIME_32,
                                           "windows_freq": list(range(1, 33)), "freq_chunks": 2}),
    "one_channel": ((24, 1, 3), "rfi", 26, {}),
    "two_channels_avg3": ((24, 2, 3), "rfi", 27, {"average_freq": 3}),
    "avg7_gt_freq": ((12, 6, 2), "rfi", 28, {"average_freq": 7, "spike_width_freq": 3.0}),
    "extends0": ((16, 48, 2), "rfi", 37, {"time_extend": 0, "freq_extend": 0}),
    "n_time_2": ((2, 64, 3), "rfi", 29, {}),
    "n_time_3": ((3, 64, 3), "rfi", 30, {"background_iterations": 2}),
    "quantised": ((24, 64, 2), "quantised", 31, {}),
    "constant_zero": ((24, 64, 3), "constant_zero", 32, {}),
    "subnormal": ((24, 64, 2), "subnormal", 33, {}),
    "large": ((24, 64, 2), "large", 34, {}),
    "negative": ((24, 64, 2), "negative", 35, {"freq_chunks": 3}),
    "nan_parts": ((24, 64, 2), "nan_parts", 36, {}),
}

#: the case whose per-baseline background and time flags are also recorded (main archive)
STAGE_CASE = "chunks1"
#: the cases whose stages are all recorded in STAGES_GOLDEN (a box radius of 32 or more in
#: wide_box)
STAGE_CASES = ["chunks1", "iter0", "wide_box", "frac_exact", "windows32", "n_time_2",
               "quantised", "subnormal", "large", "nan_parts"]  # fmt: skip
#: the reference's stages recorded for STAGE_CASES -> whether they are float32
RECORDED_STAGES = {
    "spec_flags": False, "spec_background": True, "spec_residual": True, "spec_st": False,
    "flags": False, "background": True, "residual": True, "time_flags": False,
    "freq_flags": False, "combined": False, "row_flags": False, "unaveraged": False,
}  # fmt: skip
#: the classes of edge baselines mixed into one block per input type
EDGE_KINDS = {
    False: ["quantised", "constant_zero", "subnormal", "large", "nan_parts", "nans", "rfi",
            "preflagged"],
    True: ["quantised", "constant_zero", "subnormal", "large", "negative", "amplitudes"],
}


def bandpass(n_time, n_freq, n_bl, rs):
    """A smooth bandpass with slow variation in time, float32."""
    x = np.linspace(0.0, 1.0, n_freq)
    shape = 2.0 + 0.5 * np.sin(2.5 * np.pi * x)[None, :, None]
    slope = rs.uniform(0.9, 1.1, (1, 1, n_bl)) + 0.05 * np.linspace(0, 1, n_time)[:, None, None]
    return (shape * slope).astype(np.float32)


def make_case(name):
    """(data, input_flags) of case `name`; data complex64 except for kinds 'amplitudes' and
    'negative'."""
    shape, kind, seed, _ = CASES[name]
    return make_data(shape, kind, seed)


def edge_block(shape, amplitudes, seed):
    """A block whose baselines cycle through EDGE_KINDS[amplitudes], complex64 or float32."""
    n_time, n_freq, n_bl = shape
    kinds = EDGE_KINDS[bool(amplitudes)]
    parts = [make_data((n_time, n_freq, 1), kinds[b % len(kinds)], seed + b, amplitudes)
             for b in range(n_bl)]  # fmt: skip
    return (np.concatenate([d for d, _ in parts], axis=2),
            np.concatenate([f for _, f in parts], axis=2))  # fmt: skip


def _blocks(shape, rs):
    """Flat band, little noise, interference in channels 10-13 at every time and in times
    5-6 at every channel: with single-sample windows and no smearing, exactly 4 of 32
    channels per row and 2 of 16 times per channel are flagged."""
    amp = np.full(shape, 2.0, np.float32) + (rs.standard_normal(shape) * 0.01).astype(np.float32)
    amp[:, 10:14] += 50.0
    amp[5:7] += 50.0
    return amp


def make_data(shape, kind, seed, amplitudes=None):
    """(data, input_flags) of `shape` and data class `kind`; float32 magnitudes if
    `amplitudes` (by default for the kinds 'amplitudes' and 'negative')."""
    if amplitudes is None:
        amplitudes = kind in ("amplitudes", "negative")
    n_time, n_freq, n_bl = shape
    rs = np.random.RandomState(seed=seed)
    if kind == "blocks":
        amp = _blocks(shape, rs)
        return (amp if amplitudes else amp.astype(np.complex64)), np.zeros(shape, np.bool_)
    amp = bandpass(n_time, n_freq, n_bl, rs)
    amp = amp + (rs.standard_normal(shape) * 0.1).astype(np.float32)
    flags = np.zeros(shape, np.bool_)
    if kind != "all_flagged":
        # spikes, narrow-band lines, broadband bursts and a block
        n_spikes = max(1, amp.size // 200)
        idx = tuple(rs.randint(0, s, n_spikes) for s in shape)
        amp[idx] += rs.uniform(1.0, 5.0, n_spikes).astype(np.float32)
        amp[:, rs.randint(0, n_freq, 2)] += 0.5
        amp[rs.randint(0, n_time, 1)] += 1.0
        amp[n_time // 3:n_time // 3 + 3, n_freq // 4:n_freq // 4 + 5] += 2.0
    if kind == "preflagged":
        flags[:, 10:14] = True
        flags[5] = True
        flags[:, 40:70, 0] = True
        amp[:, 10:14] = np.nan
    elif kind == "nans":
        nan_idx = tuple(rs.randint(0, s, 20) for s in shape)
        amp[nan_idx] = np.nan
        flags[rs.random_sample(shape) < 0.05] = True
    elif kind == "all_flagged":
        flags[:] = True
    elif kind == "quantised":
        # steps of 1/4: ties in every median; the phases below keep |z| exact
        amp = (np.round(amp * 4) / 4).astype(np.float32)
    elif kind == "constant_zero":
        amp[..., 0::3] = 1.5
        amp[..., 1::3] = 0.0
    elif kind == "subnormal":
        amp = amp * np.float32(1e-41)
    elif kind == "large":
        amp = amp * np.float32(1e30)
    if amplitudes:
        if kind == "negative":
            return np.where(rs.random_sample(shape) < 0.5, -amp, amp).astype(np.float32), flags
        return np.abs(amp).astype(np.float32), flags
    if kind in ("quantised", "constant_zero"):
        data = (amp * np.array([1, -1, 1j, -1j])[rs.randint(0, 4, shape)]).astype(np.complex64)
        return data, flags
    phase = rs.uniform(-np.pi, np.pi, shape)
    data = (amp * np.exp(1j * phase)).astype(np.complex64)
    if kind == "nan_parts":
        # NaN in the real part only, or in the imaginary part only
        for part in (data.real, data.imag):
            part[tuple(rs.randint(0, s, 12) for s in shape)] = np.nan
    return data, flags


def case_list():
    """JSON-friendly description of the cases (stored in the fixture and compared)."""
    return [
        {"name": name, "shape": list(shape), "kind": kind, "seed": seed, "params": params}
        for name, (shape, kind, seed, params) in sorted(CASES.items())
    ]
