"""Seeded inputs for the tests of ``rfi.host.ApplyJonesHost`` and of the device operation
(tests/test_apply_jones.py, tests/test_gpu_apply_jones.py), and the comparisons both use."""

import numpy as np

from tests.inputs_apply_gains import (  # noqa: F401  (re-exported)
    INT32_MAX,
    INT32_MIN,
    TINY,
    assert_same,
    make_flags,
    make_vis,
)

f32 = np.float32

#: antennas of the layouts (dual feed, all autocorrelations)
ANTENNAS = (1, 2, 3, 4, 17, 32)
#: baseline orders of :func:`make_inputs`
ORDERS = ("blocks", "adjacent", "random")
#: which cross products of one dish are listed: (2a, 2a+1) alone, both, neither
DISHES = ("one", "both", "neither")
#: what :func:`spoil_table` does to a table: one quad in four, the kinds in turn
SPOILS = ("drop1", "drop2", "drop4", "entry_zero", "entry_past", "entry_min", "entry_max",
          "antenna_minus", "antenna_past")  # fmt: skip


def n_quads_of(n_ant):
    return n_ant * (n_ant + 1) // 2


def make_inputs(seed, n_ant, order="blocks", dish="one"):
    """int32 (baselines, 2) for `n_ant` dual-feed antennas: the four products of every pair
    ``a < b``, the two parallel hands of every dish and, of its cross hands, what `dish` says.
    ``blocks``: one block per polarisation product, the pairs in the same order in each;
    ``adjacent``: the products of a pair next to each other; ``random``: any order and every
    baseline listed either way round, so that a table has negative entries."""
    assert order in ORDERS and dish in DISHES
    pairs = [(a, b) for a in range(n_ant) for b in range(a, n_ant)]

    def listed(a, b, m, n):
        if a != b or m == n:
            return True
        return dish == "both" or (dish == "one" and (m, n) == (0, 1))

    pols = [(0, 0), (1, 1), (0, 1), (1, 0)]
    if order == "blocks":
        inputs = [(2 * a + m, 2 * b + n) for m, n in pols for a, b in pairs if listed(a, b, m, n)]
    else:
        inputs = [(2 * a + m, 2 * b + n) for a, b in pairs for m, n in sorted(pols)
                  if listed(a, b, m, n)]  # fmt: skip
    inputs = np.array(inputs, np.int32).reshape(-1, 2)
    if order == "random":
        rs = np.random.RandomState(seed)
        inputs = inputs[rs.permutation(len(inputs))]
        swap = rs.random_sample(len(inputs)) < 0.5
        # (within a dish the other way round is the other cross hand, not the same baseline)
        swap &= inputs[:, 0] // 2 != inputs[:, 1] // 2
        inputs[swap] = inputs[swap][:, ::-1]
    return np.ascontiguousarray(inputs)


def spoil_table(seed, quad_antennas, quads, baselines, n_ant, kinds=SPOILS):
    """Copies of the two arrays in which one quad in four (at least one per kind of `kinds`,
    where there are as many quads) has one, two or all of its entries dropped (those
    baselines are then in no quad), an entry replaced by 0, ``baselines + 1``, INT32_MIN or
    INT32_MAX, or an antenna replaced by -1 or `n_ant`; the kinds take turns."""
    rs = np.random.RandomState(seed)
    quad_antennas, quads = quad_antennas.copy(), quads.copy()
    junk = {"entry_zero": 0, "entry_past": baselines + 1, "entry_min": INT32_MIN,
            "entry_max": INT32_MAX}  # fmt: skip
    chosen = rs.permutation(len(quads))[: max(len(kinds), len(quads) // 4)]
    for i, q in enumerate(chosen[: len(quads)]):
        kind = kinds[i % len(kinds)]
        if kind in ("drop1", "drop2", "drop4"):
            quads[q, rs.permutation(4)[: int(kind[4:])]] = 0
        elif kind in junk:
            quads[q, rs.randint(4)] = junk[kind]
        else:
            quad_antennas[q, rs.randint(2)] = -1 if kind == "antenna_minus" else n_ant
    return quad_antennas, quads


def covered(quads, baselines):
    """bool (baselines,): the baselines that a present entry of `quads` names."""
    t = quads.astype(np.int64).ravel()
    t = t[(t != 0) & (np.abs(t) <= baselines)]
    out = np.zeros(baselines, bool)
    out[np.abs(t) - 1] = True
    return out


#: what :func:`make_jones` puts into about 2 % of the matrices each (see there)
SPECIAL_JONES = ("nan_part", "inf", "minus_inf", "zero", "denormal", "diagonal", "singular")


def make_jones(seed, channels, n_inputs, special=True, span=10.0, leakage=0.2):
    """complex64 (channels, n_inputs, 2): diagonals of magnitude 2^U(-span, span) and any
    phase, off-diagonals up to `leakage` times the diagonal of their row. With `special`, about
    2 % of the matrices each get: a NaN in one part of one element, +inf or -inf in one part, all
    zeros, denormal elements, an exactly diagonal matrix, a singular matrix (equal rows)."""
    rs = np.random.RandomState(seed)
    shape = (channels, n_inputs)
    diagonal = np.exp2(rs.uniform(-span, span, shape)) * np.exp(1j * rs.uniform(0, 2 * np.pi, shape))
    leak = rs.uniform(0, leakage, shape) * np.exp(1j * rs.uniform(0, 2 * np.pi, shape))
    jones = np.empty((channels, n_inputs, 2), np.complex128)
    feed = np.arange(n_inputs) % 2
    rows = np.arange(n_inputs)
    jones[:, rows, feed] = diagonal
    jones[:, rows, 1 - feed] = diagonal * leak
    jones = jones.astype(np.complex64)
    if special:
        parts = jones.view(f32).reshape(channels, n_inputs // 2, 8)  # the 8 floats of a matrix
        kind = rs.random_sample(parts.shape[:2])
        part = rs.randint(0, 8, parts.shape[:2])
        for i, name in enumerate(SPECIAL_JONES):
            c, a = np.nonzero((kind >= 0.02 * i) & (kind < 0.02 * (i + 1)))
            if name == "nan_part":
                parts[c, a, part[c, a]] = np.nan
            elif name == "inf":
                parts[c, a, part[c, a]] = np.inf
            elif name == "minus_inf":
                parts[c, a, part[c, a]] = -np.inf
            elif name == "zero":
                parts[c, a, :] = 0
            elif name == "denormal":
                parts[c, a, :] = TINY * f32(3)
                parts[c, a, 1] = -TINY
            elif name == "diagonal":
                parts[c, a, 2:6] = 0
            elif name == "singular":
                parts[c, a, 4:] = parts[c, a, :4]
    return jones


def make_weights(seed, channels, baselines):
    """float32 (channels, baselines): 2^U(-10, 10) with 0, a negative weight, NaN, 2^30 and
    2^-30 in about 1 % each."""
    rs = np.random.RandomState(seed)
    shape = (channels, baselines)
    weights = np.exp2(rs.uniform(-10, 10, shape)).astype(f32)
    kind = rs.random_sample(shape)
    for i, value in enumerate([0.0, -1.5, np.nan, 2.0**30, 2.0**-30]):
        weights[(kind >= 0.01 * i) & (kind < 0.01 * (i + 1))] = value
    return weights


def make_case(seed, channels, n_ant, order="blocks", dish="one", spoil=False, flag_value=128,
              n_quads=None, extra=0):  # fmt: skip
    """dict of vis, jones, inputs, quad_antennas, quads, weights, flags for one layout, with
    `extra` baselines behind the layout's that are in no quad. `spoil`: the table goes through
    :func:`spoil_table` (True: every kind; or a tuple of kinds). `n_quads`: only the first so
    many quads of the table are kept; the baselines of the others are then in no quad."""
    from katsdpsigproc_amd.rfi import host

    inputs = make_inputs(seed, n_ant, order, dish)
    quad_antennas, quads = host.ApplyJonesHost.quad_table(inputs, 2 * n_ant)
    if extra:
        inputs = np.concatenate([inputs, np.full((extra, 2), 2 * n_ant, np.int32)])
    baselines = len(inputs)
    if n_quads is not None:
        assert n_quads <= len(quads)
        quad_antennas, quads = quad_antennas[:n_quads].copy(), quads[:n_quads].copy()
    if spoil:
        kinds = SPOILS if spoil is True else tuple(spoil)
        quad_antennas, quads = spoil_table(seed + 5, quad_antennas, quads, baselines, n_ant, kinds)
    return {
        "vis": make_vis(seed, channels, baselines),
        "jones": make_jones(seed + 1, channels, 2 * n_ant),
        "inputs": inputs,
        "quad_antennas": np.ascontiguousarray(quad_antennas, np.int32),
        "quads": np.ascontiguousarray(quads, np.int32),
        "weights": make_weights(seed + 3, channels, baselines),
        "flags": make_flags(seed + 4, channels, baselines, flag_value),
    }


def make_sparse_case(seed, channels, n_inputs, n_quads=12):
    """A few quads among many inputs: `n_quads` antenna pairs drawn from ``n_inputs / 2``
    antennas (the last antenna always among them), four products each, adjacent."""
    from katsdpsigproc_amd.rfi import host

    rs = np.random.RandomState(seed)
    n_ant = n_inputs // 2
    pairs = {(n_ant - 1, n_ant - 1), (0, n_ant - 1)}
    while len(pairs) < min(n_quads, n_quads_of(n_ant)):
        a, b = sorted(rs.randint(0, n_ant, 2))
        pairs.add((int(a), int(b)))
    inputs = np.array([(2 * a + m, 2 * b + n) for a, b in sorted(pairs) for m in range(2)
                       for n in range(2)], np.int32)  # fmt: skip
    inputs = inputs[rs.permutation(len(inputs))]
    quad_antennas, quads = host.ApplyJonesHost.quad_table(inputs, n_inputs)
    baselines = len(inputs)
    return {
        "vis": make_vis(seed, channels, baselines),
        "jones": make_jones(seed + 1, channels, n_inputs),
        "inputs": inputs,
        "quad_antennas": quad_antennas,
        "quads": quads,
        "weights": make_weights(seed + 3, channels, baselines),
        "flags": make_flags(seed + 4, channels, baselines),
    }
