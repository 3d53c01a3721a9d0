"""Solving Jones matrices without a GPU: ``rfi.host.SolveJonesHost`` against a triple loop of
float32 scalars, known answers, the referencing, the scalar solver, a float64 restatement,
argument errors, slot lists and every launch argument of every variant on the fake backend,
the sequence finalise -> solve_jones, and the argument checks of ``ksp_solve_jones``, which
come before any device call."""

import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from katsdpsigproc_amd import accel
from katsdpsigproc_amd.rfi import device, host, ingest
from tests import inputs_solve_jones as gen
from tests.fakes import FakeContext
from tests.inputs_solve_jones import assert_same

f32 = np.float32
VARIANTS = list(itertools.product([True, False], repeat=3))  # weights, flags, initial
BLOCK = 32


@pytest.fixture
def context():
    return FakeContext()


@pytest.fixture
def queue(context):
    return context.create_command_queue()


# --------------------------------------------------------------------------- the triple loop
def block_sum(terms):
    """Blocks of 32, ascending from +0 inside a block, block sums added in ascending order."""
    total = None
    for start in range(0, len(terms), BLOCK):
        partial = f32(0)
        for term in terms[start : start + BLOCK]:
            partial = f32(partial + term)
        total = partial if total is None else f32(total + partial)
    return total


def mul(a, b):
    return (f32(f32(a[0] * b[0]) - f32(a[1] * b[1])), f32(f32(a[0] * b[1]) + f32(a[1] * b[0])))


def mul_conj(a, b):
    return (f32(f32(a[0] * b[0]) + f32(a[1] * b[1])), f32(f32(a[1] * b[0]) - f32(a[0] * b[1])))


def norm2(a):
    return f32(f32(a[0] * a[0]) + f32(a[1] * a[1]))


def add(a, b):
    return (f32(a[0] + b[0]), f32(a[1] + b[1]))


def sub(a, b):
    return (f32(a[0] - b[0]), f32(a[1] - b[1]))


def csum(terms):
    return (block_sum([t[0] for t in terms]), block_sum([t[1] for t in terms]))


def triple_loop(vis, pairs, weights, flags, initial, max_iterations, tol, reference, mask,
                corrections):  # fmt: skip
    """The definition, channel by channel, element by element and step by step, in np.float32
    scalars."""
    channels, baselines = vis.shape
    n = pairs.shape[0]
    jones = np.empty((channels, n, 2), np.complex64)
    iterations = np.empty(channels, np.int32)
    status = np.empty(channels, np.uint8)
    tol2 = f32(tol * tol)
    nan, zero, one = f32(np.nan), f32(0), f32(1)
    with np.errstate(all="ignore"):
        for c in range(channels):
            a_of = [[(zero, zero)] * n for _ in range(n)]
            w_of = [[zero] * n for _ in range(n)]
            for p in range(n):
                for q in range(p + 1, n):
                    t = int(pairs[p, q])
                    if t == 0 or abs(t) > baselines or p // 2 == q // 2:
                        continue
                    j = abs(t) - 1
                    re, im = f32(vis[c, j].real), f32(vis[c, j].imag)
                    w = one if weights is None else weights[c, j]
                    if np.isnan(re) or np.isnan(im) or not w > 0:
                        continue
                    if flags is not None and int(flags[c, j]) & mask:
                        continue
                    x, y = f32(w * re), f32(w * im)
                    if t < 0:
                        y = -y
                    a_of[p][q], w_of[p][q] = (x, y), w
                    a_of[q][p], w_of[q][p] = (x, -y), w
            has = [any(w > 0 for w in row) for row in w_of]
            if initial is None:
                z = [((one, zero), (zero, zero)) if p % 2 == 0 else ((zero, zero), (one, zero))
                     for p in range(n)]  # fmt: skip
            else:
                z = [tuple((f32(initial[c, p, e].real), f32(initial[c, p, e].imag))
                           for e in range(2)) for p in range(n)]  # fmt: skip
            converged = False
            stuck = False
            k = 0
            while k < max_iterations and not converged:
                k += 1
                s00 = [norm2(x) for x, y in z]
                s11 = [norm2(y) for x, y in z]
                s01 = [mul_conj(y, x) for x, y in z]
                new = []
                stuck = False
                for p in range(n):
                    num0 = csum([mul(a_of[p][q], z[q][0]) for q in range(n)])
                    num1 = csum([mul(a_of[p][q], z[q][1]) for q in range(n)])
                    h00 = block_sum([f32(w_of[p][q] * s00[q]) for q in range(n)])
                    h11 = block_sum([f32(w_of[p][q] * s11[q]) for q in range(n)])
                    h01 = csum([(f32(w_of[p][q] * s01[q][0]), f32(w_of[p][q] * s01[q][1]))
                                for q in range(n)])  # fmt: skip
                    det = f32(f32(h00 * h11) - norm2(h01))
                    if det > 0:
                        cc, ee = mul_conj(num1, h01), mul(num0, h01)
                        new.append(((f32(f32(f32(num0[0] * h11) - cc[0]) / det),
                                     f32(f32(f32(num0[1] * h11) - cc[1]) / det)),
                                    (f32(f32(f32(num1[0] * h00) - ee[0]) / det),
                                     f32(f32(f32(num1[1] * h00) - ee[1]) / det))))  # fmt: skip
                    else:
                        new.append(z[p])
                        stuck = stuck or has[p]
                if k % 2:
                    z = new
                else:
                    old = z
                    half = f32(0.5)
                    z = [tuple((f32(f32(new[p][e][0] + old[p][e][0]) * half),
                                f32(f32(new[p][e][1] + old[p][e][1]) * half)) for e in range(2))
                         for p in range(n)]  # fmt: skip
                    d_terms, n_terms = [], []
                    for p in range(n):
                        d = f32(norm2(sub(z[p][0], old[p][0])) + norm2(sub(z[p][1], old[p][1])))
                        m = f32(norm2(z[p][0]) + norm2(z[p][1]))
                        d_terms.append(d if has[p] else zero)
                        n_terms.append(m if has[p] else zero)
                    converged = bool(block_sum(d_terms) <= f32(tol2 * block_sum(n_terms)))
            bits = (0 if converged else 1) | (0 if any(has) else 2) | (8 if stuck else 0)
            referenced = False
            if reference >= 0 and has[2 * reference] and has[2 * reference + 1]:
                (ra, rb), (rc, rd) = z[2 * reference], z[2 * reference + 1]
                big_d = sub(mul(ra, rd), mul(rb, rc))
                m = np.sqrt(norm2(big_d))
                if m > 0 and np.isfinite(m):
                    referenced = True
                    e = (f32(big_d[0] / m), f32(big_d[1] / m))
                    b00, b01 = add(ra, mul_conj(e, rd)), sub(rb, mul_conj(e, rc))
                    b10, b11 = sub(rc, mul_conj(e, rb)), add(rd, mul_conj(e, ra))
                    t = np.sqrt(np.sqrt(norm2(sub(mul(b00, b11), mul(b01, b10)))))
                    assert t.dtype == f32
                    u00, u01, u10, u11 = (
                        (f32(b[0] / t), f32(b[1] / t)) for b in (b00, b01, b10, b11))  # fmt: skip
                    z = [(add(mul_conj(x, u00), mul_conj(y, u01)),
                          add(mul_conj(x, u10), mul_conj(y, u11))) for x, y in z]  # fmt: skip
                    (x, y) = z[2 * reference]
                    z[2 * reference] = ((x[0], zero), y)
                    (x, y) = z[2 * reference + 1]
                    z[2 * reference + 1] = (x, (y[0], zero))
            bits |= 0 if referenced else 4
            for a in range(n // 2):
                rows = [z[2 * a], z[2 * a + 1]]
                if corrections:
                    (ja, jb), (jc, jd) = rows
                    big_d = sub(mul(ja, jd), mul(jb, jc))
                    s = norm2(big_d)
                    if s > 0 and has[2 * a] and has[2 * a + 1]:
                        inv = (f32(big_d[0] / s), f32(-big_d[1] / s))
                        bi, ci = mul(jb, inv), mul(jc, inv)
                        rows = [(mul(jd, inv), (-bi[0], -bi[1])), ((-ci[0], -ci[1]), mul(ja, inv))]
                    else:
                        rows = [((nan, nan), (nan, nan))] * 2
                for i in range(2):
                    row = rows[i]
                    if not corrections and not has[2 * a + i]:
                        row = ((nan, nan), (nan, nan))
                    for e in range(2):
                        jones.real[c, 2 * a + i, e], jones.imag[c, 2 * a + i, e] = row[e]
            iterations[c], status[c] = k, bits
    return jones, iterations, status


def arguments(case, weights=True, flags=True, initial=False):
    return (case["vis"], case["pairs"], case["weights"] if weights else None,
            case["flags"] if flags else None, case["initial"] if initial else None)  # fmt: skip


def assert_outputs(want, got, what=""):
    assert_same(want[0], got[0], f"jones {what}")
    for name, w, g in zip(("iterations", "status"), want[1:], got[1:]):
        assert w.dtype == g.dtype and w.shape == g.shape and (w == g).all(), (name, what, w, g)


@pytest.mark.parametrize("n_inputs, table, data, variant, settings", [
    (2, "complete", "clean", (True, True, True), (4, 1e-5, 0, 0xFF, False)),
    (4, "reversed", "hostile", (True, True, True), (5, 1e-5, 1, 0xFF, True)),
    (6, "junk", "all_flagged", (True, True, False), (6, 1e-2, 2, 0x80, False)),
    (8, "dead_feed", "hostile", (False, True, True), (7, 1e-2, -1, 0x0F, True)),
    (8, "dead_antenna", "feed1_flagged", (True, True, False), (6, 1e-5, 0, 0xFF, True)),
    (10, "isolated", "feed1_flagged", (True, True, True), (4, 1e-5, 3, 0xFF, False)),
    (34, "missing", "clean", (True, False, False), (4, 1e-2, 16, 0, True)),
    (66, "junk", "hostile", (False, False, True), (3, 0.0, 0, 0xFF, False)),
])  # fmt: skip
def test_host_against_triple_loop(n_inputs, table, data, variant, settings):
    case = gen.make_case(n_inputs, 3, n_inputs, table, data, extra=2)
    before = {name: value.copy() for name, value in case.items()}
    args = arguments(case, *variant)
    got = host.SolveJonesHost(*settings)(*args)
    want = triple_loop(*args, *settings)
    assert_outputs(want, got)
    assert all(g.flags.c_contiguous for g in got)
    for name, value in case.items():  # the inputs are never modified
        assert_same(before[name].view(np.uint8), value.view(np.uint8), name)


def test_dead_reference_and_early_stop_against_triple_loop():
    """A reference antenna with a dead feed and one with both dead, with channels free to stop
    early (tol=1e-2): not referenced, nothing rotated."""
    for table in ("dead_feed", "dead_antenna"):
        case = gen.make_case(3, 4, 12, table, "clean")
        dead = gen.dead_antenna_of(3, 12)
        settings = (60, 1e-2, dead, 0xFF, False)
        args = arguments(case)
        got = host.SolveJonesHost(*settings)(*args)
        assert_outputs(triple_loop(*args, *settings), got, table)
        assert (got[2] & 4).all() and np.isnan(got[0][:, 2 * dead + 1]).all()
        assert np.isnan(got[0][:, 2 * dead]).all() == (table == "dead_antenna")
        free = host.SolveJonesHost(60, 1e-2, -1, 0xFF, False)(*args)
        assert_same(free[0], got[0], "not rotated")


def test_generators_cover_the_cases():
    n, baselines = 40, gen.triangle(40) + 5
    upper = np.triu_indices(n, 1)
    same = upper[0] // 2 == upper[1] // 2
    for kind in gen.TABLES:
        table = gen.make_table(2, kind, n, baselines)
        assert table.dtype == np.int32 and table.shape == (n, n) and table.flags.c_contiguous
        entry = table[upper].astype(np.int64)
        named = (entry != 0) & (np.abs(entry) <= baselines)
        assert (named & same).sum() >= 10  # same-antenna entries that name real baselines
        case = gen.make_case(2, 2, n, kind, "clean", extra=5)
        junk = np.abs(case["pairs"][upper].astype(np.int64)[named & same]) - 1
        assert np.abs(case["vis"][:, junk]).min() > 1  # ... full of junk
    dead = gen.dead_antenna_of(2, n)
    for kind, silent in (("dead_feed", [2 * dead + 1]), ("dead_antenna", [2 * dead, 2 * dead + 1])):
        entry = gen.make_table(2, kind, n, baselines)[upper]
        for i in range(n):
            cross = ((upper[0] == i) | (upper[1] == i)) & ~same
            assert (entry[cross] == 0).all() == (i in silent)
    truth = gen.make_jones(3, 6, n)
    feed = np.arange(n) % 2
    diagonal = np.abs(truth[:, np.arange(n), feed])
    leak = np.abs(truth[:, np.arange(n), 1 - feed]) / diagonal
    assert diagonal.min() < 0.25 and diagonal.max() > 4 and diagonal.min() >= 0.125
    assert 0.15 < leak.max() <= 0.2 + 1e-6
    clean = gen.make_case(3, 6, n, "complete", "clean")
    table, z = clean["pairs"], clean["truth"].astype(np.complex128)
    p, q = upper[0][~same], upper[1][~same]
    model = (z[:, p] * np.conj(z[:, q])).sum(axis=2)
    assert np.abs(clean["vis"][:, table[p, q] - 1] - model).max() < 0.1
    flagged = gen.make_case(3, 6, n, "complete", "feed1_flagged")
    named_by_odd = gen.feed1_baselines(flagged["pairs"], flagged["vis"].shape[1])
    assert (flagged["flags"][-1, named_by_odd] == 0x80).all() and not flagged["flags"][:-1].any()
    hostile = gen.make_case(3, 6, n, "junk", "all_flagged", extra=5)
    assert np.isnan(hostile["vis"].real).any() and np.isinf(hostile["vis"].real).any()
    assert (hostile["flags"][-1] & 0x80).all() and np.isnan(hostile["weights"]).any()
    assert clean["initial"].shape == clean["truth"].shape == (6, n, 2)
    # the junk behind the same-antenna entries is what the host class must leave out: the
    # result with them is bit for bit the result of a table without them
    small = gen.make_case(4, 2, 8, "complete", "clean")
    entries = small["pairs"][np.arange(0, 8, 2), np.arange(1, 8, 2)]
    assert (entries > 0).all() and np.abs(small["vis"][:, entries - 1]).min() > 1
    without = small["pairs"].copy()
    without[np.arange(0, 8, 2), np.arange(1, 8, 2)] = 0
    samples = (small["weights"], small["flags"])
    assert_outputs(host.SolveJonesHost()(small["vis"], without, *samples),
                   host.SolveJonesHost()(small["vis"], small["pairs"], *samples), "same antenna")


# ------------------------------------------------------------------------- known answers
def unit_case(channels, n):
    """The data of identity matrices: 1 between equal feeds, 0 between unequal ones."""
    baselines = gen.triangle(n)
    pairs = gen.make_table(1, "complete", n, baselines)
    vis = np.zeros((channels, baselines), np.complex64)
    p, q = np.triu_indices(n, 1)
    vis[:, pairs[p, q] - 1] = (p % 2 == q % 2).astype(np.complex64)
    return vis, pairs


def identity(channels, n):
    out = np.zeros((channels, n, 2), np.complex64)
    out[:, np.arange(n), np.arange(n) % 2] = 1
    return out


@pytest.mark.parametrize("n", [4, 6, 32, 34, 70])
def test_identity_data_gives_the_identity(n):
    vis, pairs = unit_case(3, n)
    jones, iterations, status = host.SolveJonesHost()(vis, pairs)
    assert (jones == identity(3, n)).all()
    assert not np.signbit(jones.imag).any() and not np.signbit(jones.real).any()
    assert iterations.tolist() == [2] * 3 and status.tolist() == [0] * 3
    inverse = host.SolveJonesHost(corrections=True)(vis, pairs)[0]
    assert (inverse == identity(3, n)).all()
    # same-antenna entries take no part, whatever they name
    junk = vis.copy()
    junk[:, pairs[np.arange(0, n, 2), np.arange(1, n, 2)] - 1] = complex(np.nan, 1e30)
    assert_outputs((jones, iterations, status), host.SolveJonesHost()(junk, pairs))


def test_status_bits_each_alone():
    vis, pairs = unit_case(4, 6)
    flags = np.zeros(vis.shape, np.uint8)
    solve = host.SolveJonesHost
    assert solve()(vis, pairs, flags=flags)[2].tolist() == [0, 0, 0, 0]
    # bit 0: max_iterations=1 never converges
    one = solve(max_iterations=1)(vis, pairs)
    assert one[1].tolist() == [1] * 4 and one[2].tolist() == [1] * 4
    assert (one[0] == identity(4, 6)).all()
    assert solve(max_iterations=2)(vis, pairs)[2].tolist() == [0] * 4
    # bit 2: reference=-1, and a reference antenna with a dead feed
    assert solve(reference=-1)(vis, pairs)[2].tolist() == [4] * 4
    less = pairs.copy()
    less[3, :] = less[:, 3] = 0  # feed 1 of antenna 1 has no baseline
    dead = solve(reference=1)(vis, less)
    assert dead[2].tolist() == [4] * 4 and np.isnan(dead[0][:, 3]).all()
    assert (dead[0][:, [0, 1, 2, 4, 5]] == identity(4, 6)[:, [0, 1, 2, 4, 5]]).all()
    assert solve(reference=0)(vis, less)[2].tolist() == [0] * 4
    # bits 1 and 2 come together: without data nothing can be referenced
    flags[1] = 1
    none = solve()(vis, pairs, flags=flags)
    assert none[2].tolist() == [0, 2 | 4, 0, 0] and np.isnan(none[0][1]).all()
    # bit 3: every feed-1 input flagged, so H has rank 1 and det never rises above 0; the
    # feed-0 inputs keep their rows and the criterion sees no change
    flags[:] = 0
    p, q = np.triu_indices(6, 1)
    flags[2, pairs[p, q][(p % 2 == 1) | (q % 2 == 1)] - 1] = 1
    stuck = solve(reference=-1)(vis, pairs, flags=flags)
    assert stuck[2].tolist() == [4, 4, 8 | 4, 4] and stuck[1].tolist() == [2] * 4
    assert np.isnan(stuck[0][2, 1::2]).all()
    assert (stuck[0][2, 0::2] == identity(1, 6)[0, 0::2]).all()
    # (with reference=0 its antenna has a dead feed: bits 2 and 3)
    assert solve()(vis, pairs, flags=flags)[2].tolist() == [0, 0, 8 | 4, 0]
    # an infinite sample: NaN criterion, "not converged", IEEE decides the matrices
    bad = vis.copy()
    bad[0, pairs[0, 2] - 1] = complex(np.inf, 0)
    spoiled = solve(max_iterations=6)(bad, pairs)
    assert spoiled[1].tolist() == [6, 2, 2, 2] and spoiled[2][0] & 1 and not spoiled[2][1:].any()


def test_corrections_of_a_singular_matrix_are_nan():
    """Zero data: det H > 0 but num = 0, so every row becomes 0 and every det J = 0: all four
    corrections of every antenna are NaN. And an antenna with one dead feed has four NaN
    corrections, but one finite row without `corrections`."""
    vis, pairs = unit_case(2, 6)
    zero = host.SolveJonesHost(1, reference=-1, corrections=True)(np.zeros_like(vis), pairs)
    assert np.isnan(zero[0].real).all() and np.isnan(zero[0].imag).all()
    assert zero[2].tolist() == [1 | 4, 1 | 4]
    kept = host.SolveJonesHost(1, reference=-1)(np.zeros_like(vis), pairs)
    assert (kept[0] == 0).all() and kept[2].tolist() == [1 | 4, 1 | 4]
    less = pairs.copy()
    less[3, :] = less[:, 3] = 0  # feed 1 of antenna 1 has no baseline
    plain = host.SolveJonesHost()(vis, less)[0]
    inverse = host.SolveJonesHost(corrections=True)(vis, less)[0]
    assert np.isnan(plain[:, 3]).all() and (plain[:, 2] == [1, 0]).all()
    assert np.isnan(inverse[:, 2:4]).all() and (inverse[:, :2] == identity(2, 2)).all()


def matrices(jones):
    channels, n, _ = jones.shape
    return jones.astype(np.complex128).reshape(channels, n // 2, 2, 2)


def test_corrections_are_the_inverses():
    case = gen.make_case(8, 3, 14, "complete", "clean")
    jones = host.SolveJonesHost(60, 1e-6)(*arguments(case))[0]
    inverse = host.SolveJonesHost(60, 1e-6, corrections=True)(*arguments(case))[0]
    product = matrices(inverse) @ matrices(jones)
    assert np.abs(product - np.eye(2)).max() < 1e-5


# --------------------------------------------------------------------------- accuracy
def solve_float64(vis, pairs, weights, iterations, reference=0):
    """The same iteration in float64 and in matrix form, without a stopping rule, referenced
    with the unitary factor of an SVD."""
    channels, baselines = vis.shape
    n = pairs.shape[0]
    a = np.zeros((channels, n, n), np.complex128)
    w = np.zeros((channels, n, n))
    for p in range(n):
        for q in range(p + 1, n):
            t = int(pairs[p, q])
            if t == 0 or abs(t) > baselines or p // 2 == q // 2:
                continue
            v = vis[:, abs(t) - 1].astype(np.complex128)
            v = np.conj(v) if t < 0 else v
            weight = weights[:, abs(t) - 1].astype(np.float64)
            a[:, p, q], a[:, q, p] = weight * v, weight * np.conj(v)
            w[:, p, q] = w[:, q, p] = weight
    z = np.zeros((channels, n, 2), np.complex128)
    z[:, np.arange(n), np.arange(n) % 2] = 1
    for k in range(1, iterations + 1):
        num = np.einsum("cpq,cqk->cpk", a, z)
        h = np.einsum("cpq,cqj,cqk->cpjk", w, np.conj(z), z)
        det = (h[..., 0, 0] * h[..., 1, 1] - h[..., 0, 1] * h[..., 1, 0]).real
        positive = det > 0  # (elsewhere the row stays; adj(H) / det is the inverse)
        adjugate = np.stack([np.stack([h[..., 1, 1], -h[..., 0, 1]], -1),
                             np.stack([-h[..., 1, 0], h[..., 0, 0]], -1)], -2)  # fmt: skip
        inverse = adjugate / np.where(positive, det, 1.0)[..., np.newaxis, np.newaxis]
        new = np.where(positive[..., np.newaxis], np.einsum("cpj,cpjk->cpk", num, inverse), z)
        z = new if k % 2 else (new + z) / 2
    if reference >= 0:
        r = z[:, 2 * reference : 2 * reference + 2, :]
        left, _, right = np.linalg.svd(r)
        u = left @ right
        z = z @ np.conj(u.transpose(0, 2, 1))
    return z


#: the largest relative difference measured on the cases below
MEASURED_ACCURACY = 6.89e-6  # (6.882e-06 at 10 iterations, 5.178e-06 at 30)
ACCURACY_BOUND = 2 * MEASURED_ACCURACY


def accuracy_case(seed, n):
    """About 10 % of the pairs missing, except at 4 inputs: each of two antennas sees only the
    other, so one missing pair of the four leaves H with rank 1 exactly, its det is what
    rounding makes of 0, and whether a row moves is decided by the precision, not the data."""
    return gen.make_case(seed, 3, n, "complete" if n == 4 else "missing", "clean", extra=1)


@pytest.mark.parametrize("max_iterations", [10, 30])
def test_accuracy_against_float64(max_iterations):
    """tol=0 and a fixed count, so both precisions run the same iterations. Relative
    difference: the largest |z32 - z64| of a channel over its largest |z64|."""
    worst = 0.0
    for seed in gen.ACCURACY_SEEDS:
        for n in (4, 8, 34, 64):
            case = accuracy_case(seed, n)
            z32, _, status = host.SolveJonesHost(max_iterations, tol=0.0)(
                case["vis"], case["pairs"], case["weights"])  # fmt: skip
            z64 = solve_float64(case["vis"], case["pairs"], case["weights"], max_iterations)
            assert np.isfinite(z32).all() and not (status & 6).any()
            relative = np.abs(z32 - z64).max(axis=(1, 2)) / np.abs(z64).max(axis=(1, 2))
            worst = max(worst, float(relative.max()))
    print(f"largest relative difference at {max_iterations} iterations: {worst:.3e}")
    assert worst <= ACCURACY_BOUND


# --------------------------------------------------------------------------- referencing
def test_referencing():
    """After it the reference's matrix is Hermitian with a non-negative diagonal (whose
    imaginary parts are +0), and every J_a J_b^H is what it was before."""
    worst = 0.0
    for seed, n, reference in ((1, 8, 0), (2, 34, 16), (3, 64, 5)):
        case = accuracy_case(seed, n)
        args = (case["vis"], case["pairs"], case["weights"])
        free, iterations, status = host.SolveJonesHost(30, 0.0, -1)(*args)
        turned, iterations2, status2 = host.SolveJonesHost(30, 0.0, reference)(*args)
        assert (iterations == iterations2).all() and (status == status2 | 4).all()
        assert not (status2 & 4).any()
        r = matrices(turned)[:, reference]
        scale = np.abs(matrices(turned)).max(axis=(1, 2, 3))
        for i in range(2):
            imag = turned[:, 2 * reference + i, i].imag
            assert (imag == 0).all() and not np.signbit(imag).any()
            assert (turned[:, 2 * reference + i, i].real >= 0).all()
        hermitian = np.abs(r - np.conj(r.transpose(0, 2, 1))).max(axis=(1, 2)) / scale
        assert (np.linalg.eigvalsh((r + np.conj(r.transpose(0, 2, 1))) / 2) > 0).all()
        before, after = gen.products(free), gen.products(turned)
        change = np.abs(after - before).max(axis=(1, 2, 3, 4)) / np.abs(before).max(axis=(1, 2, 3, 4))
        worst = max(worst, float(hermitian.max()), float(change.max()))
    print(f"referencing: largest relative departure {worst:.3e}")
    assert worst <= ACCURACY_BOUND


# ------------------------------------------------------------------ against the scalar solver
def test_diagonals_agree_with_the_scalar_solver():
    """Data without cross-hand signal (diagonal matrices, cross-hand baselines exactly 0): the
    diagonals are what SolveGainsHost gives per feed on the parallel-hand pairs, and the
    off-diagonals stay exactly 0."""
    worst = 0.0
    for seed, n in ((1, 8), (2, 34), (3, 64)):
        baselines = gen.triangle(n) + 1
        pairs = gen.make_table(seed, "missing", n, baselines)
        truth = gen.make_jones(seed, 3, n, leakage=0.0)
        vis = gen.model_vis(seed + 1, truth, pairs, baselines)
        p, q = np.triu_indices(n, 1)
        t = pairs[p, q].astype(np.int64)
        cross_hand = (t != 0) & (p % 2 != q % 2) & (p // 2 != q // 2)
        vis[:, np.abs(t[cross_hand]) - 1] = 0
        weights = gen.make_weights(seed + 2, 3, baselines, False)
        jones = host.SolveJonesHost(30, 0.0, 1)(vis, pairs, weights)[0]
        feed = np.arange(n) % 2
        assert (jones[:, np.arange(n), 1 - feed] == 0).all()
        for i in range(2):
            sub_pairs = np.ascontiguousarray(pairs[i::2, i::2])
            gains = host.SolveGainsHost(30, 0.0, 1)(vis, sub_pairs, weights)[0]
            difference = np.abs(jones[:, i::2, i].astype(np.complex128) - gains).max(axis=1)
            worst = max(worst, float((difference / np.abs(gains).max(axis=1)).max()))
    print(f"against the scalar solver: largest relative difference {worst:.3e}")
    assert worst <= ACCURACY_BOUND


def test_converges_to_the_true_products():
    """From the identity to matrices with diagonals of 1/8 .. 8 and leakage of up to 0.2 on
    noisy data with missing pairs: J_a J_b^H at the noise level."""
    case = gen.make_case(5, 4, 48, "missing", "clean")
    jones, iterations, status = host.SolveJonesHost(200, 1e-6)(*arguments(case))
    assert not status.any() and (iterations < 200).all() and (iterations % 2 == 0).all()
    got, want = gen.products(jones), gen.products(case["truth"])
    off = ~np.eye(24, dtype=bool)
    assert np.abs(got - want)[:, off].max() / np.abs(want).max() < 2e-3  # (the noise)


# ------------------------------------------------------------------------------- errors
def test_host_errors():
    for bad in (0, 1001, -1):
        with pytest.raises(ValueError, match=r"max_iterations must be 1\.\.1000"):
            host.SolveJonesHost(max_iterations=bad)
    for bad in (1.0, True, "3"):
        with pytest.raises(TypeError, match="max_iterations"):
            host.SolveJonesHost(max_iterations=bad)
    for bad in (-1e-9, float("nan"), -np.inf):
        with pytest.raises(ValueError, match="tol"):
            host.SolveJonesHost(tol=bad)
    for bad in (-2, 64, 127, 1000):
        with pytest.raises(ValueError, match=r"reference must be -1\.\.63"):
            host.SolveJonesHost(reference=bad)
    for bad in (0.0, True):
        with pytest.raises(TypeError, match="reference"):
            host.SolveJonesHost(reference=bad)
    for bad in (-1, 256):
        with pytest.raises(ValueError, match="mask"):
            host.SolveJonesHost(mask=bad)
    with pytest.raises(TypeError, match="mask"):
        host.SolveJonesHost(mask=1.0)
    made = host.SolveJonesHost(1000, 0.0, 63, 0, 1)
    assert (made.max_iterations, made.tol, made.reference, made.mask, made.corrections) == (
        1000, 0.0, 63, 0, True)  # fmt: skip
    assert made.tol2 == 0 and made.tol2.dtype == f32
    assert host.SolveJonesHost().tol2 == f32(1e-5 * 1e-5)
    for bad in (0, 1, 3, 127, 129, 130, -2):
        with pytest.raises(ValueError, match=r"n_inputs must be even and 2\.\.128"):
            host.SolveJonesHost.check_n_inputs(bad)
    with pytest.raises(TypeError, match="n_inputs"):
        host.SolveJonesHost.check_n_inputs(4.0)
    assert host.SolveJonesHost.check_n_inputs(np.int64(128)) == 128
    with pytest.raises(ValueError, match="n_inputs must be even"):
        host.SolveJonesHost.pair_table(np.zeros((3, 2), np.int32), 5)
    fn = host.SolveJonesHost()
    good = gen.make_case(1, 4, 6, "reversed", "clean", extra=2)
    good = {name: good[name] for name in ("vis", "pairs", "weights", "flags", "initial")}
    fn(**good)
    bads = {
        "vis": [good["vis"].astype(np.complex128), good["vis"][0], np.zeros((0, 12), np.complex64),
                np.zeros((4, 0), np.complex64)],
        "pairs": [good["pairs"].astype(np.int64), good["pairs"][:4], good["pairs"][0],
                  np.zeros((0, 0), np.int32), np.zeros((5, 5), np.int32),
                  np.zeros((130, 130), np.int32)],
        "weights": [good["weights"].astype(np.float64), good["weights"][:, :5], good["weights"][0]],
        "flags": [good["flags"].astype(np.int8), good["flags"][:3], good["flags"][0]],
        "initial": [good["initial"].astype(np.complex128), good["initial"][:3],
                    good["initial"][:, :4], good["initial"][:, :, 0], good["initial"][0]],
    }  # fmt: skip
    for name, values in bads.items():
        for bad in values:
            with pytest.raises(ValueError, match=name):
                fn(**{**good, name: bad})
    with pytest.raises(ValueError, match="reference"):
        host.SolveJonesHost(reference=3)(**good)
    host.SolveJonesHost(reference=2)(**good)
    fn(good["vis"][:, :1], np.zeros((128, 128), np.int32))


def test_template_and_operation_errors(context, queue):
    with pytest.raises(ValueError):
        ingest.SolveJonesTemplate(context, tuning={"wgs": 256})
    assert ingest.SolveJonesTemplate(context, tuning={}).tuning == {}
    assert ingest.SolveJonesTemplate.autotune(context) == {}
    assert ingest.SolveJonesTemplate.host_class is host.SolveJonesHost
    assert ingest.SolveJonesTemplate.KERNEL == "ksp_solve_jones"
    assert ingest.SolveJonesTemplate.operation_class is ingest.SolveJones
    for keyword, bad, error in [
            ("max_iterations", 0, ValueError), ("max_iterations", 1001, ValueError),
            ("max_iterations", 2.0, TypeError), ("tol", -1.0, ValueError),
            ("tol", float("nan"), ValueError), ("reference", -2, ValueError),
            ("reference", 64, ValueError), ("reference", 1.5, TypeError),
            ("mask", 256, ValueError), ("mask", -1, ValueError), ("mask", 0.5, TypeError)]:  # fmt: skip
        with pytest.raises(error, match=keyword):
            ingest.SolveJonesTemplate(context, **{keyword: bad})
    template = ingest.SolveJonesTemplate(context)
    assert template.kernel.name == "ksp_solve_jones"
    assert (template.weights, template.flags, template.initial) == (True, True, False)
    assert (template.max_iterations, template.tol, template.reference, template.mask,
            template.corrections) == (30, 1e-5, 0, 0xFF, False)  # fmt: skip
    assert template.tol2 == f32(1e-10)
    for args in [(0, 4, 2), (4, 0, 2), (-4, 4, 2), (4, -1, 2), (4, 4, 0), (4, 4, -2), (4, 4, 3),
                 (4, 4, 1), (4, 4, 130)]:  # fmt: skip
        with pytest.raises(ValueError):
            template.instantiate(queue, *args)
    with pytest.raises(TypeError):
        template.instantiate(queue, 4, 4, 2.0)
    with pytest.raises(ValueError, match="reference"):
        ingest.SolveJonesTemplate(context, reference=2).instantiate(queue, 4, 4, 4)
    assert isinstance(ingest.SolveJonesTemplate(context, reference=1).instantiate(queue, 4, 4, 4),
                      ingest.SolveJones)  # fmt: skip
    assert isinstance(template.instantiate(queue, 4, 5, 128), ingest.SolveJones)
    fn = template.instantiate(queue, 1, 1, 2)
    assert fn.parameters() == {
        "weights": True, "flags": True, "initial": False, "max_iterations": 30, "tol": 1e-5,
        "reference": 0, "mask": 255, "corrections": False, "n_inputs": 2, "channels": 1,
        "baselines": 1}  # fmt: skip


def test_host_from_device(context, queue):
    case = gen.make_case(1, 4, 6, "reversed", "clean", extra=2)
    baselines = case["vis"].shape[1]
    inputs = gen.inputs_of(case["pairs"], baselines)
    for weights, flags, initial in VARIANTS:
        template = ingest.SolveJonesTemplate(context, weights=weights, flags=flags, initial=initial)
        adapter = ingest.SolveJonesHostFromDevice(template, queue)
        given = {"weights": case["weights"] if weights else None,
                 "flags": case["flags"] if flags else None,
                 "initial": case["initial"] if initial else None}  # fmt: skip
        del queue.launches[:]
        jones, iterations, status = adapter(case["vis"], inputs, 6, **given)
        assert (jones.shape, jones.dtype) == ((4, 6, 2), np.complex64)
        assert (iterations.shape, iterations.dtype) == ((4,), np.int32)
        assert (status.shape, status.dtype) == ((4,), np.uint8)
        assert [name for name, _ in queue.launches] == ["ksp_solve_jones"]
        args = queue.launches[0][1]
        assert [int(a) for a in args[8:11]] == [4, baselines, 6]
        # the table it built is what reached the pairs buffer (same-antenna entries and all:
        # the solver is what leaves them out)
        table = host.SolveGainsHost.pair_table(inputs, 6)
        assert (args[3].array[:6, :6] == table).all() and table[0, 1] != 0
        for name in ("weights", "flags", "initial"):
            wrong = dict(given)
            wrong[name] = None if given[name] is not None else case[name]
            with pytest.raises(TypeError, match=name):
                adapter(case["vis"], inputs, 6, **wrong)
    adapter = ingest.SolveJonesHostFromDevice(
        ingest.SolveJonesTemplate(context, False, False), queue)  # fmt: skip
    with pytest.raises(ValueError):
        adapter(case["vis"][0], inputs, 6)
    with pytest.raises(ValueError, match="inputs"):
        adapter(case["vis"], inputs[:-1], 6)
    for bad in (5, 130, 0):
        with pytest.raises(ValueError, match="n_inputs"):
            adapter(case["vis"], inputs, bad)
    with pytest.raises(ValueError, match="twice"):
        adapter(case["vis"], np.zeros((baselines, 2), np.int32) + [0, 1], 6)
    with pytest.raises(ValueError):
        adapter(np.zeros((0, baselines), np.complex64), inputs, 6)


# ------------------------------------------------------------------------------- wiring
def expected_slots(weights, flags, initial):
    names = ["vis"] + (["weights"] if weights else []) + (["flags"] if flags else [])
    return names + ["pairs"] + (["initial"] if initial else []) + ["jones", "iterations", "status"]


@pytest.mark.parametrize("weights, flags, initial", VARIANTS)
def test_slots(weights, flags, initial, context, queue):
    template = ingest.SolveJonesTemplate(context, weights=weights, flags=flags, initial=initial)
    fn = template.instantiate(queue, 300, 200, 20)
    assert list(fn.slots) == expected_slots(weights, flags, initial)
    shapes = {"vis": ((300, 200), np.complex64), "weights": ((300, 200), np.float32),
              "flags": ((300, 200), np.uint8), "pairs": ((20, 20), np.int32),
              "initial": ((300, 20, 2), np.complex64), "jones": ((300, 20, 2), np.complex64),
              "iterations": ((300,), np.int32), "status": ((300,), np.uint8)}  # fmt: skip
    for name, slot in fn.slots.items():
        assert (slot.shape, slot.dtype) == shapes[name], name
    # a dimension object of its own for everything that can be padded, and for the rest
    dims = [d for slot in fn.slots.values() for d in slot.dimensions]
    assert len({id(d) for d in dims}) == len(dims) == 2 * len(fn.slots) - 2 + 1 + initial
    for name in ("jones",) + (("initial",) if initial else ()):
        last = fn.slots[name].dimensions[2]
        assert last.exact and last.required_padded_size() == 2
    assert fn.parameters()["n_inputs"] == 20 and fn.parameters()["initial"] == initial


@pytest.mark.parametrize("weights, flags, initial", VARIANTS)
def test_launch_arguments(weights, flags, initial, context, queue):
    template = ingest.SolveJonesTemplate(
        context, weights=weights, flags=flags, initial=initial, max_iterations=17, tol=1e-3,
        reference=9, mask=0x41, corrections=True)  # fmt: skip
    fn = template.instantiate(queue, 300, 200, 20)
    accel.Dimension(200, min_padded_size=500).link(fn.slots["vis"].dimensions[1])
    accel.Dimension(20, min_padded_size=70).link(fn.slots["jones"].dimensions[1])
    fn()
    assert [name for name, _ in queue.launches] == ["ksp_solve_jones"]
    args = queue.launches[0][1]
    assert len(args) == 22

    def buf(name, present=True):
        return fn.buffer(name).buffer if present else None

    pointers = [buf("vis"), buf("weights", weights), buf("flags", flags), buf("pairs"),
                buf("initial", initial), buf("jones"), buf("iterations"), buf("status")]  # fmt: skip
    for got, want in zip(args[:8], pointers):
        assert got is want
    assert len({id(a) for a in args[:8] if a is not None}) == 5 + weights + flags + initial
    assert all(isinstance(a, np.int32) for a in args[8:18] + args[19:])
    assert [int(a) for a in args[8:11]] == [300, 200, 20]

    def stride(name, present=True):
        return fn.buffer(name).padded_shape[1] if present else 0

    strides = [stride("vis"), stride("weights", weights), stride("flags", flags), stride("pairs"),
               stride("initial", initial), stride("jones")]  # fmt: skip
    assert [int(a) for a in args[11:17]] == strides
    # 500 rounded up to whole 128-byte rows; the middle axis of initial and jones is not the
    # fastest, so it is padded to what is asked and no further; the last axis stays 2
    assert strides == [512, 224 if weights else 0, 256 if flags else 0, 20,
                       20 if initial else 0, 70]  # fmt: skip
    assert fn.buffer("jones").padded_shape == (300, 70, 2)
    assert int(args[17]) == 17
    assert isinstance(args[18], np.float32) and args[18] == f32(1e-3 * 1e-3)
    assert [int(a) for a in args[19:]] == [9, 0x41, 1]


def test_refining_in_place(context, queue):
    """One buffer for `initial` and `jones`."""
    fn = ingest.SolveJonesTemplate(context, initial=True).instantiate(queue, 16, 40, 10)
    fn.slots["initial"].dimensions[1].link(fn.slots["jones"].dimensions[1])
    fn.ensure_all_bound()
    fn.bind(jones=fn.buffer("initial"))
    fn()
    args = queue.launches[0][1]
    assert args[4] is args[5] is fn.buffer("initial").buffer
    assert int(args[15]) == int(args[16]) == fn.buffer("jones").padded_shape[1]


def test_behind_finalise(context, queue):
    """finalise -> solve_jones: the averaged arrays are the solver's samples, each one buffer
    with one padded size."""
    channels, baselines, cf, n_inputs = 4096, 200, 8, 20
    rows = channels // cf
    finalise = device.FinaliseTemplate(context, channel_factor=cf).instantiate(
        queue, channels, baselines)  # fmt: skip
    solve = ingest.SolveJonesTemplate(context, corrections=True).instantiate(
        queue, rows, baselines, n_inputs)  # fmt: skip
    # more row padding than either asks for, asked of one member of a compound
    accel.Dimension(baselines, min_padded_size=300).link(finalise.slots["weights"].dimensions[1])
    seq = accel.OperationSequence(
        queue, [("finalise", finalise), ("solve", solve)],
        compounds={"vis": ["finalise:vis", "solve:vis"],
                   "weights": ["finalise:weights", "solve:weights"],
                   "flags": ["finalise:flags", "solve:flags"]})  # fmt: skip
    assert {"vis", "weights", "flags", "solve:pairs", "solve:jones", "solve:iterations",
            "solve:status"} <= set(seq.slots)  # fmt: skip
    seq()
    assert [name for name, _ in queue.launches] == ["ksp_average_finalise", "ksp_solve_jones"]
    final_args, solve_args = (launch[1] for launch in queue.launches)
    assert final_args[3] is solve_args[0] is seq.buffer("vis").buffer
    assert final_args[4] is solve_args[1] is seq.buffer("weights").buffer
    assert final_args[5] is solve_args[2] is seq.buffer("flags").buffer
    assert int(final_args[14]) == int(solve_args[12]) == 320
    assert int(final_args[13]) == int(solve_args[11])
    assert int(final_args[15]) == int(solve_args[13])
    assert [int(a) for a in solve_args[8:11]] == [rows, baselines, n_inputs]
    assert int(solve_args[21]) == 1


# ------------------------------------------------------------------- the launcher's checks
@pytest.fixture(scope="module")
def lib():
    from katsdpsigproc_amd import _lib, build_native

    if not os.path.exists(_lib.LIB_PATH):
        build_native.build()
    return _lib.load()


ARRAYS = ["vis", "weights", "flags", "pairs", "initial", "jones", "iterations", "status"]
STRIDES = ["vis", "weights", "flags", "pairs", "initial", "jones"]


def test_argument_validation_without_gpu(lib):
    from katsdpsigproc_amd import _lib

    # never dereferenced: every call below fails its checks first. Eight arrays far apart.
    p = {name: ctypes.c_void_p((i + 1) << 32) for i, name in enumerate(ARRAYS)}

    def call(channels=4, baselines=8, n_inputs=4, max_iterations=30, tol2=1e-10, reference=0,
             mask=255, corrections=0, **changed):  # fmt: skip
        a = dict(p, vis_stride=8, weights_stride=8, flags_stride=8, pairs_stride=4,
                 initial_stride=4, jones_stride=4)  # fmt: skip
        a.update(changed)
        rc = lib.ksp_solve_jones(
            0, None, *(a[name] for name in ARRAYS), channels, baselines, n_inputs,
            *(a[name + "_stride"] for name in STRIDES), max_iterations, tol2, reference, mask,
            corrections)  # fmt: skip
        assert rc != 0
        return _lib.last_error()

    for name in ("vis", "pairs", "jones", "iterations", "status"):
        assert f"invalid argument: {name} is NULL" in call(**{name: None})
    for bad in (0, -1):
        assert "invalid argument: channels must be at least 1" in call(channels=bad)
        assert "invalid argument: baselines must be at least 1" in call(baselines=bad)
    for bad in (0, -2, 1, 3, 127, 129, 130):
        assert "invalid argument: n_inputs must be even and 2..128" in call(n_inputs=bad)
    for bad in (0, -1, 1001):
        assert "invalid argument: max_iterations must be 1..1000" in call(max_iterations=bad)
    for bad in (-1e-20, float("nan"), -float("inf")):
        assert "invalid argument: tol2 must be at least 0" in call(tol2=bad)
    for bad in (-2, 2, 3, 64):
        assert "invalid argument: reference must be -1..n_inputs/2-1" in call(reference=bad)
    for bad in (-1, 256):
        assert "invalid argument: mask must be 0..255" in call(mask=bad)
    for bad in (-1, 2):
        assert "invalid argument: corrections must be 0 or 1" in call(corrections=bad)
    for name in ("vis", "weights", "flags"):
        assert f"invalid argument: {name}_stride is smaller than baselines" in call(
            **{name + "_stride": 7})
    for name in ("pairs", "initial", "jones"):
        assert f"invalid argument: {name}_stride is smaller than n_inputs" in call(
            **{name + "_stride": 3})
    assert "jones_stride is smaller" in call(n_inputs=128, pairs_stride=128, initial_stride=128,
                                             jones_stride=127)  # fmt: skip
    # the order of the checks: everything wrong at once, then less and less
    strides = {name + "_stride": -1 for name in STRIDES}
    wrong = dict(channels=0, baselines=0, n_inputs=0, max_iterations=0, tol2=-1.0, reference=-2,
                 mask=-1, corrections=2)  # fmt: skip
    assert "invalid argument: vis is NULL" in call(**wrong, **dict.fromkeys(p), **strides)
    assert "invalid argument: pairs is NULL" in call(**wrong, **dict.fromkeys(p, None) | {
        "vis": p["vis"]}, **strides)  # fmt: skip
    assert "invalid argument: iterations is NULL" in call(
        **wrong, iterations=None, status=None, **strides)
    order = ["channels must", "baselines must", "n_inputs must", "max_iterations must",
             "tol2 must", "reference must", "mask must", "corrections must"]  # fmt: skip
    keys = list(wrong)
    for i, message in enumerate(order):
        assert message in call(**{key: wrong[key] for key in keys[i:]}, **strides)
    assert "invalid argument: vis_stride is smaller than baselines" in call(**strides)
    assert "invalid argument: pairs_stride is smaller than n_inputs" in call(
        **dict(strides, vis_stride=8, weights_stride=8, flags_stride=8))  # fmt: skip
    # an absent array's stride is not looked at: the call gets as far as the next check
    none = dict(weights=None, flags=None, weights_stride=0, flags_stride=0)
    assert "pairs_stride is smaller" in call(**none, pairs_stride=2)
    assert "jones_stride is smaller" in call(initial=None, initial_stride=0, jones_stride=2)

    # jones that overlaps initial without being it (a row of an input is 16 bytes)
    def at(name, offset):
        return ctypes.c_void_p(p[name].value + offset)

    message = "jones overlaps initial without being initial with the same stride"
    extent = (3 * 4 + 4) * 16  # the bytes from the first element to the last
    assert message in call(jones=at("initial", 8))
    assert message in call(jones=at("initial", extent - 1))
    assert message in call(jones=at("initial", -(extent - 1)))
    assert message in call(jones=p["initial"], jones_stride=5)  # same pointer, other stride
    # all checks pass for in place and for arrays that only touch; nothing else is left to
    # fail, so those calls are not made here (they would reach the device)
    assert message not in call(jones=at("initial", extent), n_inputs=0)


def test_header_binding_and_exports_agree(lib):
    from katsdpsigproc_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "katsdpsigproc_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declaration = re.search(r"int ksp_solve_jones\((.*?)\);", text, re.S)
    assert declaration is not None
    parameters = [" ".join(part.split()) for part in declaration.group(1).split(",")]
    argtypes = _lib.SIGNATURES["ksp_solve_jones"]
    assert len(parameters) == len(argtypes) == 24
    for parameter, argtype in zip(parameters, argtypes):
        assert ("*" in parameter) == (argtype is ctypes.c_void_p), parameter
        assert (parameter.split()[0] == "float") == (argtype is ctypes.c_float), parameter
        assert argtype in (ctypes.c_int, ctypes.c_void_p, ctypes.c_float)
    names = [parameter.replace("*", " ").split()[-1] for parameter in parameters]
    assert names == ["device", "stream"] + ARRAYS + ["channels", "baselines", "n_inputs"] + [
        name + "_stride" for name in STRIDES] + [
        "max_iterations", "tol2", "reference", "mask", "corrections"]  # fmt: skip
    assert hasattr(lib, "ksp_solve_jones")
    assert lib.ksp_abi_version() == _lib.ABI_VERSION == 5
    for name in ("SolveJonesTemplate", "SolveJones", "SolveJonesHostFromDevice"):
        assert hasattr(ingest, name)
    assert issubclass(host.SolveJonesHost, host.SolveGainsHost)
    assert host.SolveJonesHost.pair_table.__func__ is host.SolveGainsHost.pair_table.__func__
    assert host.SolveJonesHost.MAX_INPUTS == 128 and host.SolveJonesHost.BLOCK == 32
    assert host.SolveJonesHost.DET_NOT_POSITIVE == 8
