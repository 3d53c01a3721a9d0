"""Seeded inputs for the tests of ``rfi.host.SolveJonesHost`` and of the device operation
(tests/test_solve_jones.py, tests/test_gpu_solve_jones.py): model data ``J_a J_b^H`` plus
noise behind the pair tables and hostile samples of tests/inputs_solve_gains.py, and what a
leakage solve adds to them."""

import numpy as np

from tests.inputs_solve_gains import (  # noqa: F401  (re-exported)
    ACCURACY_SEEDS,
    INT32_MAX,
    INT32_MIN,
    assert_same,
    inputs_of,
    make_flags,
    make_gains,
    make_table as make_scalar_table,
    make_weights,
    triangle,
)

f32 = np.float32

#: kinds of :func:`make_table`: the scalar file's, all with same-antenna entries that name
#: real baselines, plus an antenna with one dead feed and one with both feeds dead
TABLES = ("complete", "missing", "reversed", "isolated", "junk", "dead_feed", "dead_antenna")
#: kinds of :func:`make_data`: the scalar file's, plus a last channel in which every feed-1
#: input is flagged
DATA = ("clean", "hostile", "all_flagged", "feed1_flagged")


def make_jones(seed, channels, n_inputs, span=3.0, leakage=0.2):
    """complex64 (channels, n_inputs, 2): row 2a + i is row i of antenna a's matrix; diagonals
    of magnitude 2^U(-span, span) and any phase, off-diagonals up to `leakage` times the
    diagonal of their row, any phase."""
    diagonal = make_gains(seed, channels, n_inputs, span).astype(np.complex128)
    rs = np.random.RandomState(seed + 1000)
    shape = (channels, n_inputs)
    leak = rs.uniform(0, leakage, shape) * np.exp(1j * rs.uniform(0, 2 * np.pi, shape))
    jones = np.empty((channels, n_inputs, 2), np.complex128)
    feed = np.arange(n_inputs) % 2
    rows = np.arange(n_inputs)
    jones[:, rows, feed] = diagonal
    jones[:, rows, 1 - feed] = diagonal * leak
    return jones.astype(np.complex64)


def make_table(seed, kind, n_inputs, baselines):
    """int32 (n_inputs, n_inputs) over `baselines` >= triangle(n_inputs) baselines: the scalar
    file's table of the same kind (``reversed`` for the two kinds below), in which the entries
    within one antenna name real baselines, as a caller's table may (:func:`model_vis` fills
    those with junk). ``dead_feed``: feed 1 of one antenna has no baseline; ``dead_antenna``:
    neither feed of one antenna has. `n_inputs` is even."""
    assert kind in TABLES and n_inputs % 2 == 0
    scalar = kind if kind in ("complete", "missing", "reversed", "isolated", "junk") else "reversed"
    table = make_scalar_table(seed, scalar, n_inputs, baselines).astype(np.int64)
    p, q = np.triu_indices(n_inputs, 1)
    same = p // 2 == q // 2  # (these keep the baselines of their own that the scalar table names)
    if kind in ("dead_feed", "dead_antenna") and n_inputs > 2:
        antenna = dead_antenna_of(seed, n_inputs)
        dead = [2 * antenna + 1] if kind == "dead_feed" else [2 * antenna, 2 * antenna + 1]
        for i in dead:
            cross = ((p == i) | (q == i)) & ~same
            table[p[cross], q[cross]] = 0
    return np.ascontiguousarray(table, np.int32)


def dead_antenna_of(seed, n_inputs):
    """The antenna that ``dead_feed`` and ``dead_antenna`` tables of `seed` silence."""
    return int(np.random.RandomState(seed + 3000).randint(n_inputs // 2))


def model_vis(seed, jones, table, baselines, noise=0.01):
    """complex64 (channels, baselines): ``z_p . conj(z_q)`` (or its conjugate where the table
    lists the baseline as (q, p)) plus noise of `noise` times the typical amplitude at the
    baselines that entries between antennas name; every other baseline, those that
    same-antenna entries name included, holds junk of amplitude 1e3, which a solver must never
    see."""
    rs = np.random.RandomState(seed)
    channels, n_inputs, _ = jones.shape
    shape = (channels, baselines)
    vis = 1e3 * (rs.standard_normal(shape) + 1j * rs.standard_normal(shape))
    p, q = np.triu_indices(n_inputs, 1)
    t = table[p, q].astype(np.int64)
    valid = (t != 0) & (np.abs(t) <= baselines) & (p // 2 != q // 2)
    p, q, t = p[valid], q[valid], t[valid]
    z = jones.astype(np.complex128)
    model = (z[:, p, :] * np.conj(z[:, q, :])).sum(axis=2)
    model += noise * (rs.standard_normal(model.shape) + 1j * rs.standard_normal(model.shape))
    vis[:, np.abs(t) - 1] = np.where(t < 0, np.conj(model), model)
    return vis.astype(np.complex64)


def feed1_baselines(table, baselines):
    """bool (baselines,): the baselines that a valid entry with a feed-1 (odd) input names."""
    n_inputs = table.shape[0]
    p, q = np.triu_indices(n_inputs, 1)
    t = table[p, q].astype(np.int64)
    valid = (t != 0) & (np.abs(t) <= baselines) & ((p % 2 == 1) | (q % 2 == 1))
    out = np.zeros(baselines, bool)
    out[np.abs(t[valid]) - 1] = True
    return out


def make_data(seed, kind, channels, n_inputs, table, baselines, noise=0.01):
    """dict of vis, weights, flags, initial and the true matrices. ``clean``, ``hostile`` and
    ``all_flagged`` are the scalar file's classes (hostile samples, weights and flags drawn the
    same way); ``feed1_flagged``: as ``clean``, with every baseline of a feed-1 input flagged
    (0x80) in the last channel."""
    assert kind in DATA
    hostile = kind in ("hostile", "all_flagged")
    rs = np.random.RandomState(seed + 7)
    truth = make_jones(seed, channels, n_inputs)
    vis = model_vis(seed + 1, truth, table, baselines, noise)
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
    if kind == "feed1_flagged":
        flags[-1, feed1_baselines(table, baselines)] |= 0x80
    spread = make_gains(seed + 4, channels, n_inputs, span=0.3).astype(np.complex128)
    initial = (truth * spread[:, :, np.newaxis]).astype(np.complex64)
    return {"vis": vis, "weights": make_weights(seed + 2, channels, baselines, hostile),
            "flags": flags, "initial": initial, "truth": truth}  # fmt: skip


def make_case(seed, channels, n_inputs, table="reversed", data="hostile", extra=0, noise=0.01):
    """dict of pairs, vis, weights, flags, initial, truth over triangle(n_inputs) + `extra`
    baselines."""
    baselines = triangle(n_inputs) + extra
    pairs = make_table(seed, table, n_inputs, baselines)
    case = make_data(seed + 10, data, channels, n_inputs, pairs, baselines, noise)
    case["pairs"] = pairs
    return case


def products(jones):
    """complex128 (channels, antennas, antennas, 2, 2): ``J_a J_b^H`` of complex (channels,
    n_inputs, 2) `jones`."""
    channels, n_inputs, _ = jones.shape
    j = jones.astype(np.complex128).reshape(channels, n_inputs // 2, 2, 2)
    return np.einsum("caik,cbjk->cabij", j, np.conj(j))
