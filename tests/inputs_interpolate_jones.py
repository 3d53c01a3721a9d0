"""Seeded inputs for the tests of ``rfi.host.InterpolateJonesHost`` and of the device operation
(tests/test_interpolate_jones.py, tests/test_gpu_interpolate_jones.py): tables of 2x2 matrices
of several kinds, one kind per antenna, with the per-feed delay model, the band-wide gains and
the status that go with them. The patterns of missing channels, the smooth bandpass and the
comparison are those of tests/inputs_interpolate_gains.py."""

import numpy as np

from tests import inputs_interpolate_gains as gains_gen
from tests.inputs_fit_delays import make_status
from tests.inputs_interpolate_gains import assert_same, bandpass  # noqa: F401  (re-exported)

f32 = np.float32

#: kinds whose missing channels are those of the kind of the same name in
#: tests/inputs_interpolate_gains.py (there NaN in a column, here a whole matrix NaN)
PATTERNS = ("random_holes", "none_kept", "one_kept", "first_only", "last_only", "alternating",
            "gap_exact", "gap_over", "ends", "ends_over", "runs")  # fmt: skip
#: the kinds of antenna that :func:`make_case` deals out, antenna ``a`` getting kind
#: ``KINDS[(a + first) % len(KINDS)]``
KINDS = (
    "all_kept",
    "random_holes",  # about 25 % of the channels missing, one by one
    "none_kept",
    "one_kept",
    "first_only",
    "last_only",
    "alternating",
    "gap_exact",  # gaps of exactly max_gap channels across 64, the thread count and 4096
    "gap_over",  # gaps of max_gap + 1 channels there
    "one_float",  # NaN, +inf or -inf in one of the eight floats of a matrix, each in turn
    "ends",  # max_gap channels missing at the start, max_gap + 1 at the end
    "dead_feed",  # one feed's row NaN in every channel: nothing kept
    "bad_model",  # model entries that are not finite, of either feed, kept channels or not
    "huge",  # magnitudes of 3e38
    "singular",  # second row twice the first (determinant exactly 0), some matrices all zero
    "zeros",  # every element +0 or -0: nothing to normalise by
    "diagonal",  # off-diagonal elements exactly +0
    "runs",  # runs of 1 .. 2 max_gap + 2 missing channels
    "ends_over",  # max_gap + 1 channels missing at the start, max_gap at the end
)


def make_antenna(rs, kind, channels, max_gap):
    """(matrices complex64 (channels, 2, 2), model complex64 (channels, 2)) for one antenna of
    `kind`: a bandpass per feed on the diagonal, leakage of up to 0.1 of it off the diagonal,
    every row wound by its feed's delay, which is the model."""
    c = np.arange(channels)
    matrices = np.empty((channels, 2, 2), np.complex128)
    model = np.empty((channels, 2), np.complex64)
    amplitude = np.exp2(rs.uniform(-3, 3))
    for i in range(2):
        rotation = np.exp(2j * np.pi * (c * rs.uniform(-0.3, 0.3) + rs.uniform()))
        model[:, i] = rotation
        for k in range(2):
            noise = 0.02 * (rs.standard_normal(channels) + 1j * rs.standard_normal(channels))
            smooth = bandpass(channels, rs.uniform(200, 2000)) + noise
            if i != k:
                smooth = smooth * rs.uniform(0.01, 0.1) * np.exp(2j * np.pi * rs.uniform())
            matrices[:, i, k] = amplitude * smooth * rotation
    if kind in PATTERNS:
        column, _ = gains_gen.make_column(rs, kind, channels, max_gap)
        matrices[~np.isfinite(column.view(f32).reshape(channels, 2)).all(axis=1)] = np.nan
    elif kind == "dead_feed":
        matrices[:, rs.randint(2), :] = np.nan
    elif kind == "huge":
        matrices *= 3e38 / amplitude
        matrices[rs.random_sample(channels) < 0.1] = np.nan
    elif kind == "singular":
        matrices[:, 1, :] = 2 * matrices[:, 0, :]
        matrices[rs.random_sample(channels) < 0.2] = 0
        matrices[rs.random_sample(channels) < 0.1] = np.nan
    elif kind == "zeros":
        signs = np.where(rs.random_sample((channels, 2, 2, 2)) < 0.5, 0.0, -0.0)
        matrices = signs[..., 0] + 1j * signs[..., 1]
        matrices[rs.random_sample(channels) < 0.1] = np.nan
    elif kind == "diagonal":
        matrices[:, 0, 1] = matrices[:, 1, 0] = 0
        matrices[rs.random_sample(channels) < 0.2] = np.nan
    elif kind == "bad_model":
        matrices[rs.random_sample(channels) < 0.2] = np.nan
    with np.errstate(over="ignore"):  # (huge: some parts become infinite)
        matrices = matrices.astype(np.complex64)
    if kind == "one_float":
        floats = matrices.view(f32).reshape(channels, 8)
        hit = np.flatnonzero(rs.random_sample(channels) < 0.3)
        for n, at in enumerate(hit):
            floats[at, n % 8] = (np.nan, np.inf, -np.inf)[(n // 8) % 3]
    elif kind == "bad_model":
        where = rs.random_sample(channels)
        model.real[where < 0.05, 0] = np.inf
        model.imag[(where >= 0.05) & (where < 0.1), 1] = np.nan
        model[(where >= 0.1) & (where < 0.15), 0] = complex(-np.inf, np.nan)
        model.real[(where >= 0.15) & (where < 0.2), 1] = -np.inf
    return matrices, model


def make_case(seed, channels, n_ant, max_gap, first=0, mask=0x0F, kinds=KINDS):
    """(jones, status, model, scale, kinds per antenna): complex64 (channels, 2 n_ant, 2), uint8
    (channels,) with bits inside and outside `mask`, complex64 (channels, 2 n_ant), complex64
    (2 n_ant,). One scale in eight is NaN and one is zero."""
    rs = np.random.RandomState(seed)
    n_inputs = 2 * n_ant
    jones = np.empty((channels, n_inputs, 2), np.complex64)
    model = np.empty((channels, n_inputs), np.complex64)
    names = []
    for a in range(n_ant):
        kind = kinds[(a + first) % len(kinds)]
        jones[:, 2 * a : 2 * a + 2], model[:, 2 * a : 2 * a + 2] = make_antenna(
            rs, kind, channels, max_gap)  # fmt: skip
        names.append(kind)
    scale = np.exp2(rs.uniform(-2, 2, n_inputs)) * np.exp(2j * np.pi * rs.uniform(size=n_inputs))
    scale = scale.astype(np.complex64)
    lot = rs.randint(0, 8, n_inputs)
    scale[lot == 0] = complex(np.nan, 1.0)
    scale[lot == 1] = 0
    status = make_status(seed + 1, channels, mask)
    return jones, status, model, scale, names


# ------------------------------------------------------------------------------- the chain
#: the calibrator's flagged channels: 40 in runs of at most 8, one across the wavefront's end
FLAGGED_RUNS = ((10, 8), (60, 8), (100, 5), (126, 8), (180, 3), (220, 8))
CHAIN = {"channels": 256, "n_inputs": 8, "width": 1e6, "flag_value": 0x40, "max_gap": 8,
         "max_iterations": 100, "seed": 12}  # fmt: skip
#: the largest distance of a calibrated target sample from the identity coherency that
#: :func:`chain_host` gives for CHAIN (test_host_chain_meets_its_conditions prints it); the
#: tests assert twice this
CHAIN_MEASURED = 0.00498


def chain_scan():
    """A calibrator scan and a target scan of CHAIN's 256 channels x 4 dual-feed antennas over
    all 36 baselines (autocorrelations included) with the same matrices: a bandpass per
    element, leakage of up to 0.1, a delay per feed of up to 0.02 turns per channel, the two
    feeds of the reference antenna 0 within 0.002 of each other (the per-row model leaves that
    difference on the leakage terms). The calibrator is a unit
    unpolarised source with noise of 1e-3 and 40 channels flagged and overwritten with 1e3;
    the target is unpolarised, of a flux per antenna pair, clean and noise free. A dict."""
    from katsdpsigproc_amd.rfi import host

    channels, n_inputs = CHAIN["channels"], CHAIN["n_inputs"]
    inputs = np.ascontiguousarray(np.array(np.triu_indices(n_inputs)).T, np.int32)
    baselines = len(inputs)
    rs = np.random.RandomState(CHAIN["seed"])
    c = np.arange(channels)[:, np.newaxis, np.newaxis]
    nus = rs.uniform(-0.02, 0.02, n_inputs)
    nus[1] = nus[0] + rs.uniform(-0.002, 0.002)
    shape = (n_inputs, 2)
    ripple = 1 + 0.2 * np.cos(2 * np.pi * (c / rs.uniform(200, 400, shape) + rs.uniform(size=shape)))
    leak = rs.uniform(0.02, 0.1, shape) * np.exp(2j * np.pi * rs.uniform(size=shape))
    feed = np.arange(n_inputs) % 2
    leak[np.arange(n_inputs), feed] = 1
    truth = ripple * leak * np.exp(2j * np.pi * (c * nus[:, np.newaxis] + rs.uniform(size=(n_inputs, 1))))
    p, q = inputs[:, 0], inputs[:, 1]
    response = (truth[:, p, :] * np.conj(truth[:, q, :])).sum(axis=2)
    noise = 1e-3 * (rs.standard_normal(response.shape) + 1j * rs.standard_normal(response.shape))
    cal_vis = (response + noise).astype(np.complex64)
    cal_flags = np.zeros((channels, baselines), np.uint8)
    flagged = np.zeros(channels, bool)
    for start, length in FLAGGED_RUNS:
        flagged[start : start + length] = True
    assert flagged.sum() == 40
    cal_flags[flagged] = 1
    cal_vis[flagged] = 1e3  # (what interference leaves)
    pair = (p // 2) * (n_inputs // 2) + q // 2
    sky = 2 + 0.5 * np.cos(pair)  # one flux per antenna pair: the coherency stays a multiple of I
    quad_antennas, quads = host.ApplyJonesHost.quad_table(inputs, n_inputs)
    return {"inputs": inputs, "baselines": baselines, "cal_vis": cal_vis, "cal_flags": cal_flags,
            "flagged": flagged, "target_vis": (response * sky).astype(np.complex64), "sky": sky,
            "weights": np.ones((channels, baselines), np.float32),
            "target_flags": np.zeros((channels, baselines), np.uint8),
            "pairs": host.SolveJonesHost.pair_table(inputs, n_inputs),
            "quad_antennas": quad_antennas, "quads": quads,
            "expected": (p % 2 == q % 2).astype(np.float64)}  # fmt: skip


def chain_host(scan):
    """The host classes chained as DESIGN.md section 25 chains the operations: SolveJonesHost
    -> JonesDiagonalHost -> FitDelaysHost -> InterpolateJonesHost(corrections=True) ->
    ApplyJonesHost on the target. A dict of every intermediate and final array by the name it
    has in the device sequence of tests/test_gpu_interpolate_jones.py."""
    from katsdpsigproc_amd.rfi import host

    jones, iterations, status = host.SolveJonesHost(CHAIN["max_iterations"])(
        scan["cal_vis"], scan["pairs"], scan["weights"], scan["cal_flags"])  # fmt: skip
    gains = host.JonesDiagonalHost()(jones)
    delays, phasors, amplitudes, fit_status, model = host.FitDelaysHost(CHAIN["width"])(gains, status)
    corr, kept, filled, fill_status, _ = host.InterpolateJonesHost(
        CHAIN["max_gap"], corrections=True)(jones, status, model)  # fmt: skip
    out_vis, out_weights, out_flags = host.ApplyJonesHost(CHAIN["flag_value"])(
        scan["target_vis"], corr, scan["quad_antennas"], scan["quads"], scan["weights"],
        scan["target_flags"])  # fmt: skip
    return {"jones": jones, "solve:iterations": iterations, "status": status, "gains": gains,
            "fit:delays": delays, "fit:phasors": phasors, "fit:amplitudes": amplitudes,
            "fit:fit_status": fit_status, "k": model, "corr": corr, "interp:kept": kept,
            "interp:filled": filled, "interp:fill_status": fill_status, "apply:out_vis": out_vis,
            "apply:out_weights": out_weights, "apply:out_flags": out_flags}  # fmt: skip


def chain_distance(scan, out_vis):
    """The largest |out_vis / sky - (1 on parallel hands, 0 on cross hands)| over all samples."""
    return float(np.abs(out_vis.astype(np.complex128) / scan["sky"] - scan["expected"]).max())
