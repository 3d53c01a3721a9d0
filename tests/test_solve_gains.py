"""Solving gains without a GPU: ``rfi.host.SolveGainsHost`` against a triple loop of float32
scalars, known answers and a float64 restatement, ``pair_table``, argument errors, slot lists
and every launch argument of every variant on the fake backend, the sequence finalise -> solve
-> apply_gains, and the argument checks of ``ksp_solve_gains``, which come before any device
call."""

import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from katsdpsigproc_amd import accel
from katsdpsigproc_amd.rfi import device, host, ingest
from tests import inputs_solve_gains as gen
from tests.fakes import FakeContext
from tests.inputs_solve_gains import assert_same

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


def triple_loop(vis, pairs, weights, flags, initial, max_iterations, tol, reference, mask,
                corrections):  # fmt: skip
    """The definition, channel by channel, element by element and step by step, in np.float32
    scalars."""
    channels, baselines = vis.shape
    n = pairs.shape[0]
    gains = np.empty((channels, n), np.complex64)
    iterations = np.empty(channels, np.int32)
    status = np.empty(channels, np.uint8)
    tol2 = f32(tol * tol)
    nan = f32(np.nan)
    with np.errstate(all="ignore"):
        for c in range(channels):
            a_re = [[f32(0)] * n for _ in range(n)]
            a_im = [[f32(0)] * n for _ in range(n)]
            w_of = [[f32(0)] * n for _ in range(n)]
            for p in range(n):
                for q in range(p + 1, n):
                    t = int(pairs[p, q])
                    if t == 0 or abs(t) > baselines:
                        continue
                    j = abs(t) - 1
                    re, im = f32(vis[c, j].real), f32(vis[c, j].imag)
                    w = f32(1) if weights is None else weights[c, j]
                    if np.isnan(re) or np.isnan(im) or not w > 0:
                        continue
                    if flags is not None and int(flags[c, j]) & mask:
                        continue
                    x, y = f32(w * re), f32(w * im)
                    if t < 0:
                        y = -y
                    a_re[p][q], a_im[p][q], w_of[p][q] = x, y, w
                    a_re[q][p], a_im[q][p], w_of[q][p] = x, -y, w
            has = [any(w > 0 for w in row) for row in w_of]
            if initial is None:
                g = [(f32(1), f32(0))] * n
            else:
                g = [(f32(initial[c, p].real), f32(initial[c, p].imag)) for p in range(n)]
            converged = False
            k = 0
            while k < max_iterations and not converged:
                k += 1
                s = [f32(f32(x * x) + f32(y * y)) for x, y in g]
                new = []
                for p in range(n):
                    num_re = block_sum([f32(f32(a_re[p][q] * g[q][0]) - f32(a_im[p][q] * g[q][1]))
                                        for q in range(n)])  # fmt: skip
                    num_im = block_sum([f32(f32(a_re[p][q] * g[q][1]) + f32(a_im[p][q] * g[q][0]))
                                        for q in range(n)])  # fmt: skip
                    den = block_sum([f32(w_of[p][q] * s[q]) for q in range(n)])
                    new.append((f32(num_re / den), f32(num_im / den)) if den > 0 else g[p])
                if k % 2:
                    g = new
                else:
                    old = g
                    g = [(f32(f32(x + ox) * f32(0.5)), f32(f32(y + oy) * f32(0.5)))
                         for (x, y), (ox, oy) in zip(new, old)]  # fmt: skip
                    d_terms, n_terms = [], []
                    for p in range(n):
                        dr, di = f32(g[p][0] - old[p][0]), f32(g[p][1] - old[p][1])
                        d_terms.append(f32(f32(dr * dr) + f32(di * di)) if has[p] else f32(0))
                        n_terms.append(f32(f32(g[p][0] * g[p][0]) + f32(g[p][1] * g[p][1]))
                                       if has[p] else f32(0))  # fmt: skip
                    converged = bool(block_sum(d_terms) <= f32(tol2 * block_sum(n_terms)))
            bits = (0 if converged else 1) | (0 if any(has) else 2)
            referenced = False
            if reference >= 0 and has[reference]:
                re, im = g[reference]
                m = np.sqrt(f32(f32(re * re) + f32(im * im)))
                if m > 0 and np.isfinite(m):
                    referenced = True
                    u_re, u_im = f32(re / m), f32(-im / m)
                    g = [(f32(f32(x * u_re) - f32(y * u_im)), f32(f32(x * u_im) + f32(y * u_re)))
                         for x, y in g]  # fmt: skip
                    g[reference] = (g[reference][0], f32(0))
            bits |= 0 if referenced else 4
            for p in range(n):
                x, y = g[p]
                if corrections:
                    s = f32(f32(x * x) + f32(y * y))
                    x, y = (f32(x / s), f32(-y / s)) if s > 0 else (nan, nan)
                if not has[p]:
                    x, y = nan, nan
                gains.real[c, p], gains.imag[c, p] = x, y
            iterations[c], status[c] = k, bits
    return gains, iterations, status


def arguments(case, weights=True, flags=True, initial=False):
    return (case["vis"], case["pairs"], case["weights"] if weights else None,
            case["flags"] if flags else None, case["initial"] if initial else None)  # fmt: skip


@pytest.mark.parametrize("n_inputs, table, data, variant, settings", [
    (1, "complete", "clean", (True, True, True), (4, 1e-5, 0, 0xFF, False)),
    (2, "reversed", "hostile", (True, True, True), (5, 1e-5, 1, 0xFF, True)),
    (5, "junk", "all_flagged", (True, True, False), (6, 1e-2, 4, 0x80, False)),
    (9, "isolated", "hostile", (False, True, True), (7, 1e-2, -1, 0x0F, True)),
    (33, "missing", "clean", (True, False, False), (8, 1e-2, 32, 0, True)),
    (34, "junk", "hostile", (False, False, True), (3, 0.0, 0, 0xFF, False)),
    (65, "reversed", "clean", (True, True, True), (4, 1e-3, 64, 0xFF, False)),
])  # fmt: skip
def test_host_against_triple_loop(n_inputs, table, data, variant, settings):
    case = gen.make_case(n_inputs, 3, n_inputs, table, data, extra=2)
    before = {name: value.copy() for name, value in case.items()}
    args = arguments(case, *variant)
    got = host.SolveGainsHost(*settings)(*args)
    want = triple_loop(*args, *settings)
    for name, w, g in zip(("gains", "iterations", "status"), want, got):
        if name == "gains":
            assert_same(w, g, name)
        else:
            assert w.dtype == g.dtype and (w == g).all(), (name, w, g)
        assert g.flags.c_contiguous
    for name, value in case.items():  # the inputs are never modified
        assert_same(before[name].view(np.uint8), value.view(np.uint8), name)


def test_isolated_reference_and_early_stop_against_triple_loop():
    """A reference without data, with channels free to stop early (tol=1e-2)."""
    case = gen.make_case(3, 4, 6, "isolated", "clean")
    used = np.zeros(6, bool)
    p, q = np.triu_indices(6, 1)
    valid = case["pairs"][p, q] != 0
    used[p[valid]] = used[q[valid]] = True
    lonely = int(np.flatnonzero(~used)[0])
    settings = (60, 1e-2, lonely, 0xFF, False)
    args = arguments(case)
    got = host.SolveGainsHost(*settings)(*args)
    want = triple_loop(*args, *settings)
    assert_same(want[0], got[0], "gains")
    assert (want[1] == got[1]).all() and (want[2] == got[2]).all()
    assert (got[2] & 4).all() and np.isnan(got[0][:, lonely]).all()
    assert np.isfinite(got[0][:, used]).all()


def test_generators_cover_the_cases():
    n, baselines = 40, gen.triangle(40) + 5
    upper = np.triu_indices(n, 1)
    complete = gen.make_table(1, "complete", n, baselines)[upper]
    assert (complete > 0).all() and len(set(complete.tolist())) == len(complete)
    assert complete.max() <= baselines
    missing = gen.make_table(1, "missing", n, baselines)[upper]
    assert 0.05 < np.mean(missing == 0) < 0.15 and (missing >= 0).all()
    reverse = gen.make_table(1, "reversed", n, baselines)[upper]
    assert 0.3 < np.mean(reverse < 0) < 0.6 and (reverse > 0).any()
    isolated = gen.make_table(1, "isolated", n, baselines)
    named = np.zeros(n, bool)
    valid = isolated[upper] != 0
    named[upper[0][valid]] = named[upper[1][valid]] = True
    assert (~named).sum() == 1
    junk = gen.make_table(1, "junk", n, baselines)
    for bad in (0, baselines + 1, -(baselines + 1), gen.INT32_MIN, gen.INT32_MAX):
        assert (junk[upper] == bad).any()
    for kind in gen.TABLES:
        table = gen.make_table(2, kind, n, baselines)
        assert table.dtype == np.int32 and table.shape == (n, n) and table.flags.c_contiguous
        below = table[np.tril_indices(n)]
        for bad in (gen.INT32_MIN, gen.INT32_MAX, baselines + 1):
            assert (below == bad).any()
        assert (np.abs(below.astype(np.int64)) > baselines).mean() > 0.4
    case = gen.make_case(3, 6, n, "junk", "all_flagged", extra=5)
    vis, weights, flags = case["vis"], case["weights"], case["flags"]
    assert (np.isnan(vis.real) & ~np.isnan(vis.imag)).any()
    assert (~np.isnan(vis.real) & np.isnan(vis.imag)).any()
    assert np.isposinf(vis.real).any() and np.isneginf(vis.imag).any()
    assert (weights == 0).any() and (weights < 0).any() and np.isnan(weights).any()
    assert np.isposinf(weights).any()
    assert (flags[-1] & 0x80).all() and 0.05 < np.mean(flags[:-1] != 0) < 0.15
    magnitude = np.abs(case["truth"])
    assert magnitude.min() < 0.25 and magnitude.max() > 4 and magnitude.min() >= 0.125
    clean = gen.make_case(3, 6, n, "complete", "clean")
    assert np.isfinite(clean["vis"]).all() and not clean["flags"].any()
    assert (clean["weights"] > 0).all()
    # the model: every named baseline is g_p conj(g_q) to within the noise
    table, truth = clean["pairs"], clean["truth"].astype(np.complex128)
    entry = table[upper]
    model = truth[:, upper[0]] * np.conj(truth[:, upper[1]])
    assert np.abs(clean["vis"][:, entry - 1] - model).max() < 0.1
    # inputs_of and pair_table are inverses on the valid entries
    for kind in gen.TABLES:
        table = gen.make_table(4, kind, 9, 40)
        back = host.SolveGainsHost.pair_table(gen.inputs_of(table, 40), 9)
        entry = table[np.triu_indices(9, 1)].astype(np.int64)
        want = np.where((entry != 0) & (np.abs(entry) <= 40), entry, 0)
        assert (back[np.triu_indices(9, 1)] == want).all()
        assert not back[np.tril_indices(9)].any()


# ----------------------------------------------------------------------------- pair_table
def test_pair_table():
    inputs = np.array([[0, 1], [2, 0], [1, 1], [3, 1], [-1, 2], [2, 4], [1, 2], [5, 0]], np.int32)
    table = host.SolveGainsHost.pair_table(inputs, 4)
    assert table.dtype == np.int32 and table.shape == (4, 4)
    want = np.zeros((4, 4), np.int32)
    want[0, 1], want[0, 2], want[1, 3], want[1, 2] = 1, -2, -4, 7
    assert (table == want).all()
    assert host.SolveGainsHost.pair_table(np.zeros((0, 2), np.int32), 1).tolist() == [[0]]
    assert (host.SolveGainsHost.pair_table(inputs.astype(np.int64), 4) == want).all()
    for twice in ([[0, 1], [0, 1]], [[0, 1], [2, 3], [1, 0]]):
        with pytest.raises(ValueError, match="twice"):
            host.SolveGainsHost.pair_table(np.array(twice, np.int32), 4)
    # autocorrelations and entries outside may repeat as often as they like
    host.SolveGainsHost.pair_table(np.array([[1, 1], [1, 1], [0, 9], [0, 9]], np.int32), 4)
    for bad in (0, 129, -1):
        with pytest.raises(ValueError, match=r"n_inputs must be 1\.\.128"):
            host.SolveGainsHost.pair_table(inputs, bad)
    with pytest.raises(TypeError, match="n_inputs"):
        host.SolveGainsHost.pair_table(inputs, 4.0)
    for bad in (inputs[:, 0], inputs.T, inputs.astype(np.float32), np.zeros((3, 3), np.int32)):
        with pytest.raises(ValueError, match="inputs"):
            host.SolveGainsHost.pair_table(bad, 4)
    assert host.SolveGainsHost.pair_table(inputs, 128).shape == (128, 128)


# ------------------------------------------------------------------------- known answers
def unit_case(channels, n):
    baselines = gen.triangle(n)
    return np.ones((channels, baselines), np.complex64), gen.make_table(1, "complete", n, baselines)


@pytest.mark.parametrize("n", [2, 3, 32, 33, 70])
def test_unit_data_gives_unit_gains(n):
    vis, pairs = unit_case(3, n)
    gains, iterations, status = host.SolveGainsHost()(vis, pairs)
    assert (gains == 1).all() and not np.signbit(gains.imag).any()
    assert iterations.tolist() == [2] * 3 and status.tolist() == [0] * 3
    corrections = host.SolveGainsHost(corrections=True)(vis, pairs)[0]
    assert (corrections.real == 1).all() and (corrections.imag == 0).all()


def test_scaled_unit_data():
    """vis = 4 on every baseline: gains of 2, reached to rounding from unit gains."""
    vis, pairs = unit_case(2, 6)
    gains, iterations, status = host.SolveGainsHost(100, 1e-6)(vis * f32(4), pairs)
    assert np.abs(gains - 2).max() < 1e-5 and not status.any() and (iterations % 2 == 0).all()
    weighted = host.SolveGainsHost(100, 1e-6)(vis * f32(4), pairs, np.full(vis.shape, 8, f32))
    assert np.abs(weighted[0] - 2).max() < 1e-5


def test_no_data_input_is_nan_and_the_others_are_unaffected():
    vis, pairs = unit_case(2, 5)
    vis = (vis * f32(4)).astype(np.complex64)
    less = pairs.copy()
    less[:, 4] = 0  # input 4 has no baseline
    got = host.SolveGainsHost(40, 1e-6)(vis, less)
    # (the 4 x 4 corner of the table names the same baselines of the same array)
    small = host.SolveGainsHost(40, 1e-6)(vis, np.ascontiguousarray(pairs[:4, :4]))
    assert np.isnan(got[0][:, 4].real).all() and np.isnan(got[0][:, 4].imag).all()
    assert_same(small[0], np.ascontiguousarray(got[0][:, :4]), "the other inputs")
    assert (got[1] == small[1]).all() and not got[2].any()
    # NaN samples, zero weights and flags leave an input out just as well
    for spoil in ("nan", "weight", "flag"):
        v, w, f = vis.copy(), np.ones(vis.shape, f32), np.zeros(vis.shape, np.uint8)
        column = np.abs(pairs[:4, 4]) - 1
        if spoil == "nan":
            v[:, column] = complex(0, np.nan)
        elif spoil == "weight":
            w[:, column] = [0, -1, np.nan, -0.0]
        else:
            f[:, column] = [1, 2, 0x80, 0xFF]
        again = host.SolveGainsHost(40, 1e-6)(v, pairs, w, f)
        assert_same(got[0], again[0], spoil)
    # a mask that ignores the flags brings the input back
    f = np.zeros(vis.shape, np.uint8)
    f[:, np.abs(pairs[:4, 4]) - 1] = 0x10
    assert np.isnan(host.SolveGainsHost(mask=0x10)(vis, pairs, flags=f)[0][:, 4]).all()
    assert np.isfinite(host.SolveGainsHost(mask=0xEF)(vis, pairs, flags=f)[0]).all()


def test_status_bits_and_reference():
    vis, pairs = unit_case(3, 4)
    flags = np.zeros(vis.shape, np.uint8)
    flags[1] = 1  # a channel with everything flagged
    gains, iterations, status = host.SolveGainsHost()(vis, pairs, flags=flags)
    assert status.tolist() == [0, 2 | 4, 0] and iterations.tolist() == [2, 2, 2]
    assert np.isnan(gains[1]).all() and (gains[[0, 2]] == 1).all()
    # reference=-1: nothing is turned, and bit 2 says so
    initial = np.full((3, 4), np.exp(0.7j), np.complex64)
    free = host.SolveGainsHost(reference=-1)(vis, pairs, initial=initial)
    assert free[2].tolist() == [4, 4, 4] and np.abs(np.angle(free[0]) - 0.7).max() < 1e-6
    for reference in range(4):
        fixed = host.SolveGainsHost(reference=reference)(vis, pairs, initial=initial)
        assert not fixed[2].any()
        assert (fixed[0][:, reference].imag == 0).all()
        assert not np.signbit(fixed[0][:, reference].imag).any()
        assert np.abs(fixed[0] - 1).max() < 1e-6
    # a reference without data, and one whose gain is zero: not referenced, gains untouched
    less = pairs.copy()
    less[0, :] = 0
    lonely = host.SolveGainsHost(reference=0)(vis, less, initial=initial)
    assert lonely[2].tolist() == [4, 4, 4] and np.isnan(lonely[0][:, 0]).all()
    assert np.abs(np.angle(lonely[0][:, 1:]) - 0.7).max() < 1e-6
    zero = host.SolveGainsHost(reference=0)(np.zeros_like(vis), pairs)
    assert (zero[2] & 4).all() and (zero[0] == 0).all()
    # max_iterations=1 never converges, 2 can
    one = host.SolveGainsHost(max_iterations=1)(vis, pairs)
    assert one[1].tolist() == [1, 1, 1] and one[2].tolist() == [1, 1, 1] and (one[0] == 1).all()
    assert host.SolveGainsHost(max_iterations=2)(vis, pairs)[2].tolist() == [0, 0, 0]
    # an infinite sample: NaN criterion, "not converged", IEEE decides the gains
    bad = vis.copy()
    bad[0, 0] = complex(np.inf, 0)
    spoiled = host.SolveGainsHost(max_iterations=6)(bad, pairs)
    assert spoiled[1].tolist() == [6, 2, 2] and spoiled[2][0] & 1 and not spoiled[2][1:].any()


def test_corrections():
    """conj(g) / |g|^2 of the referenced gains, and NaN where |g|^2 underflows to 0."""
    case = gen.make_case(8, 3, 7, "complete", "clean")
    gains = host.SolveGainsHost(60, 1e-6)(*arguments(case))[0]
    inverse = host.SolveGainsHost(60, 1e-6, corrections=True)(*arguments(case))[0]
    s = gains.real * gains.real + gains.imag * gains.imag
    assert_same(gains.real / s, np.ascontiguousarray(inverse.real), "re")
    assert_same(-gains.imag / s, np.ascontiguousarray(inverse.imag), "im")
    assert np.abs(gains * inverse - 1).max() < 1e-6
    # one baseline of 1e-30 and gains (1, 1e-30), which solve it: input 0's divisor underflows,
    # so it keeps its gain, and input 1 gets 1e-30 / 1
    vis = np.full((1, 1), 1e-30, np.complex64)
    pairs = np.array([[0, 1], [0, 0]], np.int32)
    start = np.array([[1, 1e-30]], np.complex64)
    plain = host.SolveGainsHost(2, tol=0.0, reference=-1)(vis, pairs, initial=start)
    assert plain[0][0, 0] == 1 and plain[0][0, 1] == f32(1e-30)
    assert plain[1].tolist() == [2] and plain[2].tolist() == [4]
    inverse = host.SolveGainsHost(2, tol=0.0, reference=-1, corrections=True)(
        vis, pairs, initial=start)[0]  # fmt: skip
    assert inverse[0, 0] == 1
    assert np.isnan(inverse[0, 1].real) and np.isnan(inverse[0, 1].imag)
    # without data the answer is NaN whatever the gain
    none = host.SolveGainsHost(1, corrections=True)(vis, np.zeros_like(pairs), initial=start)
    assert np.isnan(none[0]).all() and none[2].tolist() == [1 | 2 | 4]


# ------------------------------------------------------------------------------ accuracy
def solve_float64(vis, pairs, weights, iterations):
    """The same iteration in float64 and in matrix form, without a stopping rule, referenced
    to input 0."""
    channels, baselines = vis.shape
    n = pairs.shape[0]
    a = np.zeros((channels, n, n), np.complex128)
    w = np.zeros((channels, n, n))
    for p in range(n):
        for q in range(p + 1, n):
            t = int(pairs[p, q])
            if t == 0 or abs(t) > baselines:
                continue
            v = vis[:, abs(t) - 1].astype(np.complex128)
            v = np.conj(v) if t < 0 else v
            weight = weights[:, abs(t) - 1].astype(np.float64)
            a[:, p, q], a[:, q, p] = weight * v, weight * np.conj(v)
            w[:, p, q] = w[:, q, p] = weight
    g = np.ones((channels, n), np.complex128)
    for k in range(1, iterations + 1):
        new = np.einsum("cpq,cq->cp", a, g) / np.einsum("cpq,cq->cp", w, np.abs(g) ** 2)
        g = new if k % 2 else (new + g) / 2
    return g * (np.conj(g[:, :1]) / np.abs(g[:, :1]))


#: the largest relative difference measured on the cases below
MEASURED_ACCURACY = 6.05e-7


@pytest.mark.parametrize("max_iterations", [10, 30])
def test_accuracy_against_float64(max_iterations):
    """tol=0 and a fixed count, so both precisions run the same iterations (a float32 run that
    stops early has d == 0 exactly: it no longer moves). Relative difference: the largest
    |g32 - g64| of a channel over its largest |g64|."""
    worst = 0.0
    for seed in gen.ACCURACY_SEEDS:
        for n in (3, 8, 33, 64):
            case = gen.make_case(seed, 3, n, "missing", "clean", extra=1)
            g32 = host.SolveGainsHost(max_iterations, tol=0.0)(
                case["vis"], case["pairs"], case["weights"])[0]  # fmt: skip
            g64 = solve_float64(case["vis"], case["pairs"], case["weights"], max_iterations)
            assert np.isfinite(g32).all()
            relative = np.abs(g32 - g64).max(axis=1) / np.abs(g64).max(axis=1)
            worst = max(worst, float(relative.max()))
    print(f"largest relative difference at {max_iterations} iterations: {worst:.3e}")
    assert worst <= 2 * MEASURED_ACCURACY


def test_converges_to_the_true_gains():
    """From unit gains to gains of magnitude 1/8 .. 8 on noisy data with missing pairs."""
    case = gen.make_case(5, 4, 48, "missing", "clean")
    gains, iterations, status = host.SolveGainsHost(200, 1e-6)(*arguments(case))
    assert not status.any() and (iterations < 200).all() and (iterations % 2 == 0).all()
    truth = case["truth"].astype(np.complex128)
    truth = truth * np.conj(truth[:, :1]) / np.abs(truth[:, :1])
    assert np.abs(gains - truth).max() / np.abs(truth).max() < 2e-3  # (the noise, not rounding)


# ------------------------------------------------------------------------------- errors
def test_host_errors():
    for bad in (0, 1001, -1):
        with pytest.raises(ValueError, match=r"max_iterations must be 1\.\.1000"):
            host.SolveGainsHost(max_iterations=bad)
    for bad in (1.0, True, "3"):
        with pytest.raises(TypeError, match="max_iterations"):
            host.SolveGainsHost(max_iterations=bad)
    for bad in (-1e-9, float("nan"), -np.inf):
        with pytest.raises(ValueError, match="tol"):
            host.SolveGainsHost(tol=bad)
    for bad in (-2, 128, 1000):
        with pytest.raises(ValueError, match=r"reference must be -1\.\.127"):
            host.SolveGainsHost(reference=bad)
    with pytest.raises(TypeError, match="reference"):
        host.SolveGainsHost(reference=0.0)
    for bad in (-1, 256):
        with pytest.raises(ValueError, match="mask"):
            host.SolveGainsHost(mask=bad)
    with pytest.raises(TypeError, match="mask"):
        host.SolveGainsHost(mask=1.0)
    made = host.SolveGainsHost(1000, 0.0, 127, 0, 1)
    assert (made.max_iterations, made.tol, made.reference, made.mask, made.corrections) == (
        1000, 0.0, 127, 0, True)  # fmt: skip
    assert made.tol2 == 0 and made.tol2.dtype == f32
    assert host.SolveGainsHost().tol2 == f32(1e-5 * 1e-5)
    fn = host.SolveGainsHost()
    good = gen.make_case(1, 4, 5, "reversed", "clean", extra=2)
    good = {name: good[name] for name in ("vis", "pairs", "weights", "flags", "initial")}
    fn(**good)
    bads = {
        "vis": [good["vis"].astype(np.complex128), good["vis"][0], np.zeros((0, 12), np.complex64),
                np.zeros((4, 0), np.complex64)],
        "pairs": [good["pairs"].astype(np.int64), good["pairs"][:4], good["pairs"][0],
                  np.zeros((0, 0), np.int32), np.zeros((129, 129), np.int32)],
        "weights": [good["weights"].astype(np.float64), good["weights"][:, :5], good["weights"][0]],
        "flags": [good["flags"].astype(np.int8), good["flags"][:3], good["flags"][0]],
        "initial": [good["initial"].astype(np.complex128), good["initial"][:3],
                    good["initial"][:, :4], good["initial"][0]],
    }  # fmt: skip
    for name, values in bads.items():
        for bad in values:
            with pytest.raises(ValueError, match=name):
                fn(**{**good, name: bad})
    with pytest.raises(ValueError, match="reference"):
        host.SolveGainsHost(reference=5)(**good)
    host.SolveGainsHost(reference=4)(**good)
    fn(good["vis"][:, :1], np.zeros((128, 128), np.int32))


def test_template_and_operation_errors(context, queue):
    with pytest.raises(ValueError):
        ingest.SolveGainsTemplate(context, tuning={"wgs": 256})
    assert ingest.SolveGainsTemplate(context, tuning={}).tuning == {}
    assert ingest.SolveGainsTemplate.autotune(context) == {}
    assert ingest.SolveGainsTemplate.host_class is host.SolveGainsHost
    assert ingest.SolveGainsTemplate.KERNEL == "ksp_solve_gains"
    assert ingest.SolveGainsTemplate.operation_class is ingest.SolveGains
    for keyword, bad, error in [
            ("max_iterations", 0, ValueError), ("max_iterations", 1001, ValueError),
            ("max_iterations", 2.0, TypeError), ("tol", -1.0, ValueError),
            ("tol", float("nan"), ValueError), ("reference", -2, ValueError),
            ("reference", 128, ValueError), ("reference", 1.5, TypeError),
            ("mask", 256, ValueError), ("mask", -1, ValueError), ("mask", 0.5, TypeError)]:  # fmt: skip
        with pytest.raises(error, match=keyword):
            ingest.SolveGainsTemplate(context, **{keyword: bad})
    template = ingest.SolveGainsTemplate(context)
    assert template.kernel.name == "ksp_solve_gains"
    assert (template.weights, template.flags, template.initial) == (True, True, False)
    assert (template.max_iterations, template.tol, template.reference, template.mask,
            template.corrections) == (30, 1e-5, 0, 0xFF, False)  # fmt: skip
    assert template.tol2 == f32(1e-10)
    for args in [(0, 4, 2), (4, 0, 2), (-4, 4, 2), (4, -1, 2), (4, 4, 0), (4, 4, -1), (4, 4, 129)]:
        with pytest.raises(ValueError):
            template.instantiate(queue, *args)
    with pytest.raises(ValueError, match="reference"):
        ingest.SolveGainsTemplate(context, reference=3).instantiate(queue, 4, 4, 3)
    assert isinstance(ingest.SolveGainsTemplate(context, reference=2).instantiate(queue, 4, 4, 3),
                      ingest.SolveGains)  # fmt: skip
    assert isinstance(template.instantiate(queue, 4, 5, 128), ingest.SolveGains)
    fn = template.instantiate(queue, 1, 1, 1)
    assert fn.parameters() == {
        "weights": True, "flags": True, "initial": False, "max_iterations": 30, "tol": 1e-5,
        "reference": 0, "mask": 255, "corrections": False, "n_inputs": 1, "channels": 1,
        "baselines": 1}  # fmt: skip


def test_host_from_device(context, queue):
    case = gen.make_case(1, 4, 5, "reversed", "clean", extra=2)
    baselines = case["vis"].shape[1]
    inputs = gen.inputs_of(case["pairs"], baselines)
    for weights, flags, initial in VARIANTS:
        template = ingest.SolveGainsTemplate(context, weights=weights, flags=flags, initial=initial)
        adapter = ingest.SolveGainsHostFromDevice(template, queue)
        given = {"weights": case["weights"] if weights else None,
                 "flags": case["flags"] if flags else None,
                 "initial": case["initial"] if initial else None}  # fmt: skip
        del queue.launches[:]
        gains, iterations, status = adapter(case["vis"], inputs, 5, **given)
        assert (gains.shape, gains.dtype) == ((4, 5), np.complex64)
        assert (iterations.shape, iterations.dtype) == ((4,), np.int32)
        assert (status.shape, status.dtype) == ((4,), np.uint8)
        assert [name for name, _ in queue.launches] == ["ksp_solve_gains"]
        args = queue.launches[0][1]
        assert [int(a) for a in args[8:11]] == [4, baselines, 5]
        # the table it built is what reached the pairs buffer
        table = host.SolveGainsHost.pair_table(inputs, 5)
        assert (args[3].array[:5, :5] == table).all()
        for name in ("weights", "flags", "initial"):
            wrong = dict(given)
            wrong[name] = None if given[name] is not None else case[name]
            with pytest.raises(TypeError, match=name):
                adapter(case["vis"], inputs, 5, **wrong)
    adapter = ingest.SolveGainsHostFromDevice(
        ingest.SolveGainsTemplate(context, False, False), queue)  # fmt: skip
    with pytest.raises(ValueError):
        adapter(case["vis"][0], inputs, 5)
    with pytest.raises(ValueError, match="inputs"):
        adapter(case["vis"], inputs[:-1], 5)
    with pytest.raises(ValueError, match="n_inputs"):
        adapter(case["vis"], inputs, 129)
    with pytest.raises(ValueError, match="twice"):
        adapter(case["vis"], np.zeros((baselines, 2), np.int32) + [0, 1], 5)
    with pytest.raises(ValueError):
        adapter(np.zeros((0, baselines), np.complex64), inputs, 5)


# ------------------------------------------------------------------------------- wiring
def expected_slots(weights, flags, initial):
    names = ["vis"] + (["weights"] if weights else []) + (["flags"] if flags else [])
    return names + ["pairs"] + (["initial"] if initial else []) + ["gains", "iterations", "status"]


@pytest.mark.parametrize("weights, flags, initial", VARIANTS)
def test_slots(weights, flags, initial, context, queue):
    template = ingest.SolveGainsTemplate(context, weights=weights, flags=flags, initial=initial)
    fn = template.instantiate(queue, 300, 200, 20)
    assert list(fn.slots) == expected_slots(weights, flags, initial)
    shapes = {"vis": ((300, 200), np.complex64), "weights": ((300, 200), np.float32),
              "flags": ((300, 200), np.uint8), "pairs": ((20, 20), np.int32),
              "initial": ((300, 20), np.complex64), "gains": ((300, 20), np.complex64),
              "iterations": ((300,), np.int32), "status": ((300,), np.uint8)}  # fmt: skip
    for name, slot in fn.slots.items():
        assert (slot.shape, slot.dtype) == shapes[name], name
    # a dimension object of its own for everything that can be padded
    dims = [d for slot in fn.slots.values() for d in slot.dimensions]
    assert len({id(d) for d in dims}) == len(dims) == 2 * len(fn.slots) - 2
    assert fn.parameters()["n_inputs"] == 20 and fn.parameters()["initial"] == initial


@pytest.mark.parametrize("weights, flags, initial", VARIANTS)
def test_launch_arguments(weights, flags, initial, context, queue):
    template = ingest.SolveGainsTemplate(
        context, weights=weights, flags=flags, initial=initial, max_iterations=17, tol=1e-3,
        reference=19, mask=0x41, corrections=True)  # fmt: skip
    fn = template.instantiate(queue, 300, 200, 20)
    accel.Dimension(200, min_padded_size=500).link(fn.slots["vis"].dimensions[1])
    accel.Dimension(20, min_padded_size=70).link(fn.slots["gains"].dimensions[1])
    fn()
    assert [name for name, _ in queue.launches] == ["ksp_solve_gains"]
    args = queue.launches[0][1]
    assert len(args) == 22

    def buf(name, present=True):
        return fn.buffer(name).buffer if present else None

    pointers = [buf("vis"), buf("weights", weights), buf("flags", flags), buf("pairs"),
                buf("initial", initial), buf("gains"), buf("iterations"), buf("status")]  # fmt: skip
    for got, want in zip(args[:8], pointers):
        assert got is want
    assert len({id(a) for a in args[:8] if a is not None}) == 5 + weights + flags + initial
    assert all(isinstance(a, np.int32) for a in args[8:18] + args[19:])
    assert [int(a) for a in args[8:11]] == [300, 200, 20]

    def stride(name, present=True):
        return fn.buffer(name).padded_shape[1] if present else 0

    strides = [stride("vis"), stride("weights", weights), stride("flags", flags), stride("pairs"),
               stride("initial", initial), stride("gains")]  # fmt: skip
    assert [int(a) for a in args[11:17]] == strides
    # 500 and 70 rounded up to whole 128-byte rows; the others as their own slots ask (a row
    # of `pairs` is shorter than 128 bytes and stays as it is)
    assert strides == [512, 224 if weights else 0, 256 if flags else 0, 20,
                       32 if initial else 0, 80]  # fmt: skip
    assert int(args[17]) == 17
    assert isinstance(args[18], np.float32) and args[18] == f32(1e-3 * 1e-3)
    assert [int(a) for a in args[19:]] == [19, 0x41, 1]


def test_refining_in_place(context, queue):
    """One buffer for `initial` and `gains`."""
    fn = ingest.SolveGainsTemplate(context, initial=True).instantiate(queue, 16, 40, 9)
    fn.slots["initial"].dimensions[1].link(fn.slots["gains"].dimensions[1])
    fn.ensure_all_bound()
    fn.bind(gains=fn.buffer("initial"))
    fn()
    args = queue.launches[0][1]
    assert args[4] is args[5] is fn.buffer("initial").buffer
    assert int(args[15]) == int(args[16]) == fn.buffer("gains").padded_shape[1]


def test_between_finalise_and_apply_gains(context, queue):
    """finalise -> solve -> apply_gains: the averaged arrays are the samples of both, each one
    buffer with one padded size, and the solver's `gains` are the `gains` that are applied."""
    channels, baselines, cf, n_inputs = 4096, 200, 8, 20
    rows = channels // cf
    finalise = device.FinaliseTemplate(context, channel_factor=cf).instantiate(
        queue, channels, baselines)  # fmt: skip
    solve = ingest.SolveGainsTemplate(context, corrections=True).instantiate(
        queue, rows, baselines, n_inputs)  # fmt: skip
    apply_gains = ingest.ApplyGainsTemplate(context).instantiate(queue, rows, baselines, n_inputs)
    # more row padding than any of them asks for, asked of one member of each compound
    accel.Dimension(baselines, min_padded_size=300).link(finalise.slots["weights"].dimensions[1])
    accel.Dimension(n_inputs, min_padded_size=100).link(apply_gains.slots["gains"].dimensions[1])
    seq = accel.OperationSequence(
        queue, [("finalise", finalise), ("solve", solve), ("apply_gains", apply_gains)],
        compounds={"vis": ["finalise:vis", "solve:vis", "apply_gains:vis"],
                   "weights": ["finalise:weights", "solve:weights", "apply_gains:weights"],
                   "flags": ["finalise:flags", "solve:flags", "apply_gains:flags"],
                   "gains": ["solve:gains", "apply_gains:gains"]})  # fmt: skip
    assert {"vis", "weights", "flags", "gains", "solve:pairs", "solve:iterations", "solve:status",
            "apply_gains:inputs", "apply_gains:out_vis"} <= set(seq.slots)  # fmt: skip
    seq()
    assert [name for name, _ in queue.launches] == [
        "ksp_average_finalise", "ksp_solve_gains", "ksp_apply_gains"]  # fmt: skip
    final_args, solve_args, apply_args = (launch[1] for launch in queue.launches)
    assert final_args[3] is solve_args[0] is apply_args[0] is seq.buffer("vis").buffer
    assert final_args[4] is solve_args[1] is apply_args[1] is seq.buffer("weights").buffer
    assert final_args[5] is solve_args[2] is apply_args[2] is seq.buffer("flags").buffer
    assert solve_args[5] is apply_args[3] is seq.buffer("gains").buffer
    assert int(final_args[14]) == int(solve_args[12]) == int(apply_args[12]) == 320
    assert int(final_args[13]) == int(solve_args[11]) == int(apply_args[11])
    assert int(final_args[15]) == int(solve_args[13]) == int(apply_args[13])
    assert int(solve_args[16]) == int(apply_args[14]) == seq.buffer("gains").padded_shape[1] == 112
    assert [int(a) for a in solve_args[8:11]] == [rows, baselines, n_inputs]
    assert int(solve_args[21]) == 1


# ------------------------------------------------------------------- the launcher's checks
@pytest.fixture(scope="module")
def lib():
    from katsdpsigproc_amd import _lib, build_native

    if not os.path.exists(_lib.LIB_PATH):
        build_native.build()
    return _lib.load()


ARRAYS = ["vis", "weights", "flags", "pairs", "initial", "gains", "iterations", "status"]
STRIDES = ["vis", "weights", "flags", "pairs", "initial", "gains"]


def test_argument_validation_without_gpu(lib):
    from katsdpsigproc_amd import _lib

    # never dereferenced: every call below fails its checks first. Eight arrays far apart.
    p = {name: ctypes.c_void_p((i + 1) << 32) for i, name in enumerate(ARRAYS)}

    def call(channels=4, baselines=8, n_inputs=3, max_iterations=30, tol2=1e-10, reference=0,
             mask=255, corrections=0, **changed):  # fmt: skip
        a = dict(p, vis_stride=8, weights_stride=8, flags_stride=8, pairs_stride=3,
                 initial_stride=3, gains_stride=3)  # fmt: skip
        a.update(changed)
        rc = lib.ksp_solve_gains(
            0, None, *(a[name] for name in ARRAYS), channels, baselines, n_inputs,
            *(a[name + "_stride"] for name in STRIDES), max_iterations, tol2, reference, mask,
            corrections)  # fmt: skip
        assert rc != 0
        return _lib.last_error()

    for name in ("vis", "pairs", "gains", "iterations", "status"):
        assert f"invalid argument: {name} is NULL" in call(**{name: None})
    for bad in (0, -1):
        assert "invalid argument: channels must be at least 1" in call(channels=bad)
        assert "invalid argument: baselines must be at least 1" in call(baselines=bad)
    for bad in (0, -1, 129):
        assert "invalid argument: n_inputs must be 1..128" in call(n_inputs=bad)
    for bad in (0, -1, 1001):
        assert "invalid argument: max_iterations must be 1..1000" in call(max_iterations=bad)
    for bad in (-1e-20, float("nan"), -float("inf")):
        assert "invalid argument: tol2 must be at least 0" in call(tol2=bad)
    for bad in (-2, 3, 128):
        assert "invalid argument: reference must be -1..n_inputs-1" in call(reference=bad)
    for bad in (-1, 256):
        assert "invalid argument: mask must be 0..255" in call(mask=bad)
    for bad in (-1, 2):
        assert "invalid argument: corrections must be 0 or 1" in call(corrections=bad)
    for name in ("vis", "weights", "flags"):
        assert f"invalid argument: {name}_stride is smaller than baselines" in call(
            **{name + "_stride": 7})
    for name in ("pairs", "initial", "gains"):
        assert f"invalid argument: {name}_stride is smaller than n_inputs" in call(
            **{name + "_stride": 2})
    assert "gains_stride is smaller" in call(n_inputs=128, pairs_stride=128, initial_stride=128,
                                             gains_stride=127)  # fmt: skip
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
    assert "gains_stride is smaller" in call(initial=None, initial_stride=0, gains_stride=2)

    # gains that overlap initial without being it
    def at(name, offset):
        return ctypes.c_void_p(p[name].value + offset)

    message = "gains overlaps initial without being initial with the same stride"
    extent = (3 * 3 + 3) * 8  # the bytes from the first element to the last
    assert message in call(gains=at("initial", 8))
    assert message in call(gains=at("initial", extent - 1))
    assert message in call(gains=at("initial", -(extent - 1)))
    assert message in call(gains=p["initial"], gains_stride=4)  # same pointer, other stride
    # all checks pass for in place and for arrays that only touch; nothing else is left to
    # fail, so those calls are not made here (they would reach the device)
    assert message not in call(gains=at("initial", extent), n_inputs=0)


def test_header_binding_and_exports_agree(lib):
    from katsdpsigproc_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "katsdpsigproc_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declaration = re.search(r"int ksp_solve_gains\((.*?)\);", text, re.S)
    assert declaration is not None
    parameters = [" ".join(part.split()) for part in declaration.group(1).split(",")]
    argtypes = _lib.SIGNATURES["ksp_solve_gains"]
    assert len(parameters) == len(argtypes) == 24
    for parameter, argtype in zip(parameters, argtypes):
        assert ("*" in parameter) == (argtype is ctypes.c_void_p), parameter
        assert (parameter.split()[0] == "float") == (argtype is ctypes.c_float), parameter
        assert argtype in (ctypes.c_int, ctypes.c_void_p, ctypes.c_float)
    names = [parameter.replace("*", " ").split()[-1] for parameter in parameters]
    assert names == ["device", "stream"] + ARRAYS + ["channels", "baselines", "n_inputs"] + [
        name + "_stride" for name in STRIDES] + [
        "max_iterations", "tol2", "reference", "mask", "corrections"]  # fmt: skip
    assert hasattr(lib, "ksp_solve_gains")
    assert lib.ksp_abi_version() == _lib.ABI_VERSION == 5
    for name in ("SolveGainsTemplate", "SolveGains", "SolveGainsHostFromDevice"):
        assert hasattr(ingest, name)
    assert hasattr(host, "SolveGainsHost")
    assert host.SolveGainsHost.MAX_INPUTS == 128 and host.SolveGainsHost.BLOCK == 32
