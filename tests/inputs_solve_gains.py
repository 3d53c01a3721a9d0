"""Seeded inputs for the tests of ``rfi.host.SolveGainsHost`` and of the device operation
(tests/test_solve_gains.py, tests/test_gpu_solve_gains.py): model data ``g_a conj(g_b)`` plus
noise behind pair tables of several kinds, hostile samples, and the comparison both use."""

import numpy as np

from tests.inputs_apply_gains import assert_same  # noqa: F401  (re-exported)

f32 = np.float32
INT32_MIN, INT32_MAX = -(2**31), 2**31 - 1

#: kinds of :func:`make_table`
TABLES = ("complete", "missing", "reversed", "isolated", "junk")
#: kinds of :func:`make_data`
DATA = ("clean", "hostile", "all_flagged")
#: the seeds the accuracy test runs on
ACCURACY_SEEDS = (1, 2, 3)


def triangle(n_inputs):
    """Baselines of a full triangle without autocorrelations."""
    return n_inputs * (n_inputs - 1) // 2


def make_gains(seed, channels, n_inputs, span=3.0):
    """complex64 (channels, n_inputs): magnitudes 2^U(-span, span), any phase."""
    rs = np.random.RandomState(seed)
    shape = (channels, n_inputs)
    magnitude = np.exp2(rs.uniform(-span, span, shape))
    phase = rs.uniform(0, 2 * np.pi, shape)
    return (magnitude * np.exp(1j * phase)).astype(np.complex64)


def make_table(seed, kind, n_inputs, baselines):
    """int32 (n_inputs, n_inputs) over `baselines` >= triangle(n_inputs) baselines: the pairs
    p < q scattered over the baselines in a random order. ``complete``: every pair, listed as
    (p, q); ``missing``: about 10 % of the pairs 0; ``reversed``: about half listed as (q, p)
    (t < 0), 10 % missing; ``isolated``: as ``reversed``, and one input has no baseline at
    all; ``junk``: as ``reversed``, with 0, baselines + 1, -(baselines + 1), INT32_MIN and
    INT32_MAX in about 3 % of the pairs each. Every kind has junk on the diagonal and below
    it, which nothing may read."""
    assert kind in TABLES and baselines >= triangle(n_inputs)
    rs = np.random.RandomState(seed)
    table = rs.randint(INT32_MIN, INT32_MAX, (n_inputs, n_inputs), dtype=np.int64)
    lower = np.tril_indices(n_inputs)
    extremes = np.array([INT32_MIN, INT32_MAX, 1, -1, baselines, baselines + 1, 0])
    table[lower] = np.where(rs.random_sample(len(lower[0])) < 0.5,
                            extremes[rs.randint(0, len(extremes), len(lower[0]))], table[lower])  # fmt: skip
    p, q = np.triu_indices(n_inputs, 1)
    entry = rs.permutation(baselines)[: len(p)].astype(np.int64) + 1
    kind_of = rs.random_sample(len(p))
    if kind != "complete":
        entry[kind_of < 0.1] = 0
    if kind in ("reversed", "isolated", "junk"):
        entry = np.where(rs.random_sample(len(p)) < 0.5, -entry, entry)
    if kind == "isolated" and n_inputs > 1:
        lonely = rs.randint(n_inputs)
        entry[(p == lonely) | (q == lonely)] = 0
    if kind == "junk":
        for i, bad in enumerate([0, baselines + 1, -(baselines + 1), INT32_MIN, INT32_MAX]):
            entry[(kind_of >= 0.1 + 0.03 * i) & (kind_of < 0.13 + 0.03 * i)] = bad
    table[p, q] = entry
    return np.ascontiguousarray(table, np.int32)


def model_vis(seed, gains, table, baselines, noise=0.01):
    """complex64 (channels, baselines): ``g_p conj(g_q)`` (or its conjugate where the table
    lists the baseline as (q, p)) plus noise of `noise` times the typical amplitude; baselines
    the table does not name hold noise of amplitude 1e3, which a solver must never see."""
    rs = np.random.RandomState(seed)
    channels, n_inputs = gains.shape
    shape = (channels, baselines)
    vis = 1e3 * (rs.standard_normal(shape) + 1j * rs.standard_normal(shape))
    p, q = np.triu_indices(n_inputs, 1)
    t = table[p, q].astype(np.int64)
    valid = (t != 0) & (np.abs(t) <= baselines)
    p, q, t = p[valid], q[valid], t[valid]
    g = gains.astype(np.complex128)
    model = g[:, p] * np.conj(g[:, q])
    model += noise * (rs.standard_normal(model.shape) + 1j * rs.standard_normal(model.shape))
    vis[:, np.abs(t) - 1] = np.where(t < 0, np.conj(model), model)
    return vis.astype(np.complex64)


def make_weights(seed, channels, baselines, hostile):
    """float32 (channels, baselines): 2^U(-2, 2) and, `hostile`, 0, negative, -0 and NaN in
    about 2 % each, and +inf likewise but in the second channel only."""
    rs = np.random.RandomState(seed)
    shape = (channels, baselines)
    weights = np.exp2(rs.uniform(-2, 2, shape)).astype(f32)
    if hostile:
        kind = rs.random_sample(shape)
        for i, value in enumerate([0.0, -1.5, -0.0, np.nan, np.inf]):
            where = (kind >= 0.02 * i) & (kind < 0.02 * (i + 1))
            if np.isinf(value):
                where[:1] = where[2:] = False  # (see make_data)
            weights[where] = value
    return weights


def make_flags(seed, channels, baselines, hostile):
    """uint8 (channels, baselines): zero but for about 10 % random non-zero bytes."""
    rs = np.random.RandomState(seed)
    shape = (channels, baselines)
    flags = np.zeros(shape, np.uint8)
    if hostile:
        some = rs.random_sample(shape) < 0.1
        flags[some] = rs.randint(1, 256, shape).astype(np.uint8)[some]
    return flags


def make_data(seed, kind, channels, n_inputs, table, baselines):
    """dict of vis, weights, flags, initial and the true gains. ``clean``: model data, benign
    weights, no flags; ``hostile``: NaN in one part and +-0 in about 1 % of the samples each,
    +-inf likewise but in the second channel only (one infinity leaves a channel nothing but
    NaN gains), hostile weights and flags; ``all_flagged``: as ``hostile``, with the last
    channel flagged throughout (0x80)."""
    assert kind in DATA
    hostile = kind != "clean"
    rs = np.random.RandomState(seed + 7)
    truth = make_gains(seed, channels, n_inputs)
    vis = model_vis(seed + 1, truth, table, baselines)
    if hostile:
        sample = rs.random_sample(vis.shape)
        specials = [complex(np.nan, 1), complex(1, np.nan), complex(np.inf, 1), complex(1, -np.inf),
                    complex(0.0, -0.0), complex(np.nan, np.nan)]  # fmt: skip
        for i, value in enumerate(specials):
            where = (sample >= 0.01 * i) & (sample < 0.01 * (i + 1))
            if np.isinf(value.real) or np.isinf(value.imag):
                where[:1] = where[2:] = False  # (an infinity leaves a channel nothing but NaN)
            vis[where] = value
    flags = make_flags(seed + 3, channels, baselines, hostile)
    if kind == "all_flagged":
        flags[-1] |= 0x80
    initial = (truth * make_gains(seed + 4, channels, n_inputs, span=0.3)).astype(np.complex64)
    return {"vis": vis, "weights": make_weights(seed + 2, channels, baselines, hostile),
            "flags": flags, "initial": initial, "truth": truth}  # fmt: skip


def make_case(seed, channels, n_inputs, table="reversed", data="hostile", extra=0):
    """dict of pairs, vis, weights, flags, initial, truth over triangle(n_inputs) + `extra`
    baselines (at least 1)."""
    baselines = max(1, triangle(n_inputs) + extra)
    pairs = make_table(seed, table, n_inputs, baselines)
    case = make_data(seed + 10, data, channels, n_inputs, pairs, baselines)
    case["pairs"] = pairs
    return case


def inputs_of(table, baselines):
    """The ApplyGains-style int32 (baselines, 2) that ``pair_table`` turns back into the valid
    entries of `table`; baselines the table does not name are autocorrelations of input 0."""
    n_inputs = table.shape[0]
    inputs = np.zeros((baselines, 2), np.int32)
    p, q = np.triu_indices(n_inputs, 1)
    t = table[p, q].astype(np.int64)
    valid = (t != 0) & (np.abs(t) <= baselines)
    for a, b, entry in zip(p[valid], q[valid], t[valid]):
        inputs[abs(entry) - 1] = (a, b) if entry > 0 else (b, a)
    return inputs
