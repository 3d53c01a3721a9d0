"""Seeded inputs of the 2-D SumThreshold flagger cases, shared by
``golden/make_golden_twodflag.py`` and the tests that check against its fixture."""

import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "rfi_twodflag_golden.npz")  # fmt: skip

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
}

#: the case whose per-baseline background and time flags are also recorded
STAGE_CASE = "chunks1"


def bandpass(n_time, n_freq, n_bl, rs):
    """A smooth bandpass with slow variation in time, float32."""
    x = np.linspace(0.0, 1.0, n_freq)
    shape = 2.0 + 0.5 * np.sin(2.5 * np.pi * x)[None, :, None]
    slope = rs.uniform(0.9, 1.1, (1, 1, n_bl)) + 0.05 * np.linspace(0, 1, n_time)[:, None, None]
    return (shape * slope).astype(np.float32)


def make_case(name):
    """(data, input_flags) of case `name`; data complex64 except for kind 'amplitudes'."""
    shape, kind, seed, _ = CASES[name]
    n_time, n_freq, n_bl = shape
    rs = np.random.RandomState(seed=seed)
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
    if kind == "amplitudes":
        return np.abs(amp).astype(np.float32), flags
    phase = rs.uniform(-np.pi, np.pi, shape)
    data = (amp * np.exp(1j * phase)).astype(np.complex64)
    return data, flags


def case_list():
    """JSON-friendly description of the cases (stored in the fixture and compared)."""
    return [
        {"name": name, "shape": list(shape), "kind": kind, "seed": seed, "params": params}
        for name, (shape, kind, seed, params) in sorted(CASES.items())
    ]
