"""``rfi.host.InterpolateJonesHost`` and ``rfi.host.JonesDiagonalHost`` (the definitions)
against a loop of float32 scalars and against known answers, the wiring of
``rfi.ingest.InterpolateJonesTemplate`` and ``rfi.ingest.JonesDiagonalTemplate`` on the fake
backend, and the checks of ``ksp_interpolate_jones`` and ``ksp_jones_diagonal``, which run
before any device call. Nothing here needs a GPU; tests/test_gpu_interpolate_jones.py compares
the kernels with the host classes."""

import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from katsdpsigproc_amd import accel
from katsdpsigproc_amd.rfi import host, ingest
from tests import inputs_interpolate_gains as gains_gen
from tests import inputs_interpolate_jones as gen
from tests.fakes import FakeContext
from tests.inputs_interpolate_jones import assert_same

f32 = np.float32
NAN = complex(np.nan, np.nan)
#: (status, model, scale, normalise, corrections) of every variant of the operation
VARIANTS = list(itertools.product([True, False], repeat=5))
OUTPUTS = ("out", "kept", "filled", "fill_status", "mean_amplitude")
NO_DATA, GAP_LEFT = 1, 2


@pytest.fixture
def context():
    return FakeContext()


@pytest.fixture
def queue(context):
    return context.create_command_queue()


# ----------------------------------------------------------------------------- the scalar loop
def scalar_tree(terms):
    n = len(terms)
    terms = list(terms)
    while n > 1:
        n //= 2
        for i in range(n):
            terms[i] = terms[i] + terms[i + n]
    return terms[0]


def mul(a, b):
    return (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])


def finite(pair):
    return bool(np.isfinite(pair[0]) and np.isfinite(pair[1]))


def scalar_antenna(z, status, m, scale, max_gap, smooth, normalise, mask, corrections):
    """One antenna: `z` a list per channel of four (float32, float32) in the order 00, 01, 10,
    11; `m` a list per channel of two pairs (or None); `status` a list of ints (or None);
    `scale` two pairs (or None). Returns (out as `z`, kept, filled, fill_status,
    mean_amplitude or None)."""
    channels = len(z)
    nan = f32(np.nan)
    kept, s = [], []
    for c in range(channels):
        ok = all(finite(x) for x in z[c])
        if status is not None:
            ok = ok and (status[c] & mask) == 0
        if m is not None:
            ok = ok and finite(m[c][0]) and finite(m[c][1])
            s.append([(x[0] * m[c][e // 2][0] + x[1] * m[c][e // 2][1],
                       x[1] * m[c][e // 2][0] - x[0] * m[c][e // 2][1])
                      for e, x in enumerate(z[c])])  # fmt: skip
        else:
            s.append(list(z[c]))
        kept.append(ok)
    n_kept = sum(kept)
    failed = n_kept == 0
    if smooth > 1:
        reach = smooth // 2
        smoothed = [list(x) for x in s]
        for c in range(channels):
            if not kept[c]:
                continue
            for e in range(4):
                re, im, n = f32(0), f32(0), 0
                for j in range(max(0, c - reach), min(channels - 1, c + reach) + 1):
                    if kept[j]:
                        re, im, n = re + s[j][e][0], im + s[j][e][1], n + 1
                smoothed[c][e] = (re / f32(n), im / f32(n))
        s = smoothed
    mean_amplitude = None
    if normalise:
        c_pad = 1
        while c_pad < channels:
            c_pad *= 2
        terms = [f32(0)] * c_pad
        for c in range(channels):
            if kept[c]:
                n00, n01, n10, n11 = (x[0] * x[0] + x[1] * x[1] for x in s[c])
                terms[c] = np.sqrt(((n00 + n01) + (n10 + n11)) * f32(0.5))
        mean_amplitude = scalar_tree(terms) / f32(n_kept) if n_kept else nan
        if mean_amplitude > 0 and mean_amplitude < np.inf:
            s = [[(x[0] / mean_amplitude, x[1] / mean_amplitude) for x in row] for row in s]
        else:
            failed = True
    out, filled, gap_left = [], 0, False
    for c in range(channels):
        if failed:
            out.append([(nan, nan)] * 4)
            continue
        if kept[c]:
            y = list(s[c])
        else:
            below = [j for j in range(c) if kept[j]]
            above = [j for j in range(c + 1, channels) if kept[j]]
            y = None
            if below and above:
                l, r = below[-1], above[0]
                if r - l - 1 <= max_gap:
                    t = f32(c - l) / f32(r - l)
                    y = [tuple(s[l][e][i] + (s[r][e][i] - s[l][e][i]) * t for i in range(2))
                         for e in range(4)]  # fmt: skip
            elif below:
                if c - below[-1] <= max_gap:
                    y = list(s[below[-1]])
            elif above[0] - c <= max_gap:
                y = list(s[above[0]])
            if y is None:
                y = [(nan, nan)] * 4
                gap_left = True
            else:
                filled += 1
        if m is not None:
            y = [mul(x, m[c][e // 2]) for e, x in enumerate(y)]
        if scale is not None:
            y = [mul(x, scale[e // 2]) for e, x in enumerate(y)]
        if corrections:
            ja, jb, jc, jd = y
            ad, bc = mul(ja, jd), mul(jb, jc)
            big_d = (ad[0] - bc[0], ad[1] - bc[1])
            q = big_d[0] * big_d[0] + big_d[1] * big_d[1]
            if q > 0:
                inv = (big_d[0] / q, -big_d[1] / q)
                bi, ci = mul(jb, inv), mul(jc, inv)
                y = [mul(jd, inv), (-bi[0], -bi[1]), (-ci[0], -ci[1]), mul(ja, inv)]
            else:
                y = [(nan, nan)] * 4
        assert all(type(part) is f32 for x in y for part in x)
        out.append(y)
    bits = NO_DATA if failed else GAP_LEFT if gap_left else 0
    return out, n_kept, filled, bits, mean_amplitude


def scalar_loop(jones, status, model, scale, max_gap, smooth, normalise, mask, corrections):
    def pair(v):
        return (f32(v.real), f32(v.imag))

    channels, n_inputs, _ = jones.shape
    n_ant = n_inputs // 2
    out = np.empty(jones.shape, np.complex64)
    kept, filled = np.empty(n_ant, np.int32), np.empty(n_ant, np.int32)
    fill_status = np.empty(n_ant, np.uint8)
    mean_amplitude = np.empty(n_ant, f32) if normalise else None
    with np.errstate(all="ignore"):
        for a in range(n_ant):
            z = [[pair(jones[c, 2 * a + i, k]) for i in (0, 1) for k in (0, 1)]
                 for c in range(channels)]  # fmt: skip
            m = None if model is None else [
                [pair(model[c, 2 * a]), pair(model[c, 2 * a + 1])] for c in range(channels)]
            sc = None if scale is None else [pair(scale[2 * a]), pair(scale[2 * a + 1])]
            rows, kept[a], filled[a], fill_status[a], amplitude = scalar_antenna(
                z, None if status is None else [int(v) for v in status], m, sc,
                max_gap, smooth, normalise, mask, corrections)  # fmt: skip
            for c, row in enumerate(rows):
                for e, y in enumerate(row):
                    out[c, 2 * a + e // 2, e % 2] = complex(y[0], y[1])
                    # (complex() of two float32 and the store round nothing: both are exact)
            if normalise:
                mean_amplitude[a] = amplitude
    return out, kept, filled, fill_status, mean_amplitude


def check(want, got, what=""):
    assert len(want) == len(got) == 5
    for name, w, g in zip(OUTPUTS, want, got):
        if w is None:
            assert g is None, name
        else:
            assert_same(w, g, f"{name} {what}")


def pick(case, variant):
    """(status, model, scale) of make_case's result, None for what `variant` leaves out."""
    return tuple(a if wanted else None for a, wanted in zip(case[1:4], variant))


@pytest.mark.parametrize("channels, max_gap, smooth, variant", [
    (1, 1, 1, (True, True, True, True, True)), (2, 0, 3, (False, True, False, True, False)),
    (3, 2, 1, (True, False, True, False, True)), (37, 3, 5, (True, True, True, True, True)),
    (64, 4, 31, (False, False, False, True, False)), (65, 1, 1, (False, False, False, False, False)),
    (130, 8, 9, (True, True, False, False, True)), (100, 16384, 3, (False, True, True, True, False)),
])  # fmt: skip
def test_host_against_scalar_loop(channels, max_gap, smooth, variant):
    normalise, corrections = variant[3:]
    case = gen.make_case(channels + smooth, channels, len(gen.KINDS) + 2, max_gap)
    jones, args = case[0], pick(case, variant)
    before = [None if a is None else a.copy() for a in (jones,) + args]
    got = host.InterpolateJonesHost(max_gap, smooth, normalise, 0x0F, corrections)(jones, *args)
    want = scalar_loop(jones, *args, max_gap, smooth, normalise, 0x0F, corrections)
    check(want, got, f"at {channels}, {variant}")
    for b, a in zip(before, (jones,) + args):  # no argument is modified
        assert b is None or (b.view(np.uint8) == a.view(np.uint8)).all()
    assert not np.shares_memory(got[0], jones)


def test_generators_cover_the_cases():
    """Across the kinds, every outcome occurs: both status bits, filled and unfilled channels,
    a whole matrix going missing for one float, a dead feed, matrices that cannot be inverted
    and an amplitude that cannot be normalised by."""
    jones, status, model, scale, kinds = gen.make_case(5, 300, len(gen.KINDS), 4)
    assert tuple(kinds) == gen.KINDS
    at = dict(zip(kinds, range(len(kinds))))
    out, kept, filled, bits, amplitude = host.InterpolateJonesHost(4, 3, True)(jones, None, model)
    assert set(bits.tolist()) == {0, NO_DATA, GAP_LEFT}
    assert kept[at["all_kept"]] == 300 and filled[at["all_kept"]] == 0
    for kind in ("none_kept", "dead_feed", "zeros"):
        assert bits[at[kind]] == NO_DATA and filled[at[kind]] == 0, kind
        assert np.isnan(out[:, 2 * at[kind] : 2 * at[kind] + 2]).all()
    assert kept[at["none_kept"]] == kept[at["dead_feed"]] == 0 and kept[at["zeros"]] > 0
    assert np.isnan(amplitude[at["dead_feed"]]) and amplitude[at["zeros"]] == 0
    assert bits[at["gap_exact"]] == 0 and bits[at["gap_over"]] == GAP_LEFT
    assert kept[at["one_kept"]] == kept[at["first_only"]] == kept[at["last_only"]] == 1
    # one float of eight that is not finite takes the whole matrix with it
    a = at["one_float"]
    floats = jones[:, 2 * a : 2 * a + 2].reshape(300, 4).view(f32)
    spoilt = ~np.isfinite(floats)
    assert (spoilt.sum(axis=1) <= 1).all() and spoilt.any(axis=0).all()
    assert kept[a] == 300 - spoilt.any(axis=1).sum() < 300
    a = at["bad_model"]
    assert kept[a] < np.isfinite(jones[:, 2 * a : 2 * a + 2]).all(axis=(1, 2)).sum()
    # a singular matrix is kept and filled, and has no inverse
    a = at["singular"]
    inverse = host.InterpolateJonesHost(4, corrections=True)(jones)
    assert inverse[3][a] == 0 and np.isnan(inverse[0][:, 2 * a : 2 * a + 2]).all()
    assert np.isfinite(inverse[0][:, 0:2]).all()
    # the status has bits inside and outside the mask, and only those inside count
    assert (status & 0x0F).any() and (status & 0xF0).any()
    with_status = host.InterpolateJonesHost(4, status_mask=0x0F)(jones, status)
    assert with_status[1][0] == 300 - np.count_nonzero(status & 0x0F)


# ------------------------------------------------------------------------- the consequences
def test_identity_on_kept_channels():
    jones, status, _, _, kinds = gen.make_case(9, 257, len(gen.KINDS), 3)
    out, kept, _, bits, _ = host.InterpolateJonesHost(3, status_mask=0x0F)(jones, status)
    n_ant = len(kinds)
    ok = np.isfinite(jones.reshape(257, n_ant, 4)).all(axis=2) & ((status & 0x0F) == 0)[:, np.newaxis]
    assert (ok.sum(axis=0) == kept).all()
    alive = bits != NO_DATA
    assert (alive == (kept > 0)).all() and alive.sum() >= n_ant - 4
    same = (out.view(np.uint64) == jones.view(np.uint64)).reshape(257, n_ant, 4).all(axis=2)
    assert same[ok & alive].all()
    assert np.isnan(out.reshape(257, n_ant, 4)[:, ~alive]).all()


@pytest.mark.parametrize("smooth, with_model, with_scale", [(1, False, False), (5, True, True),
                                                            (31, True, False), (3, False, True)])  # fmt: skip
def test_diagonal_matrices_are_interpolate_gains(smooth, with_model, with_scale):
    """Exactly diagonal matrices whose feeds share their kept channels: the diagonal of `out` is
    InterpolateGainsHost's `out` for the two inputs bit for bit, the counts are the inputs',
    and the off-diagonal elements stay zero (NaN where the diagonal is NaN)."""
    channels, n_inputs, max_gap = 200, 12, 3
    kinds = ("random_holes", "runs", "all_kept", "ends", "gap_over", "huge")
    gains, status, model, scale, _ = gains_gen.make_case(3, channels, n_inputs, max_gap, kinds=kinds)
    gains = gains.copy()
    missing = ~np.isfinite(gains.view(f32).reshape(channels, n_inputs, 2)).all(axis=2)
    both = missing[:, 0::2] | missing[:, 1::2]
    gains[np.repeat(both, 2, axis=1)] = NAN
    jones = np.zeros((channels, n_inputs, 2), np.complex64)
    feed = np.arange(n_inputs) % 2
    jones[:, np.arange(n_inputs), feed] = gains
    args = (status, model if with_model else None, scale if with_scale else None)
    want = host.InterpolateGainsHost(max_gap, smooth, status_mask=0x0F)(gains, *args)
    got = host.InterpolateJonesHost(max_gap, smooth, status_mask=0x0F)(jones, *args)
    assert_same(want[0], host.JonesDiagonalHost()(got[0]), "the diagonal")
    for w, g in zip(want[1:4], got[1:4]):
        assert (w[0::2] == g).all() and (w[1::2] == g).all()
    assert set(got[3].tolist()) <= {0, GAP_LEFT} and (got[2] > 0).all()
    off = got[0][:, np.arange(n_inputs), 1 - feed]
    diagonal_nan = np.isnan(want[0].real) | np.isnan(want[0].imag)
    held = ~np.isnan(off.real) & ~np.isnan(off.imag)
    assert (off[held] == 0).all()
    assert (held | diagonal_nan | ~np.isfinite(np.where(with_scale, scale, 1))[np.newaxis]).all()


def test_constant_matrix_comes_back_constant():
    value = np.array([[1.5 - 2j, 0.25j], [-0.125, 3 + 0.5j]], np.complex64)
    jones = np.tile(value, (40, 3, 1))
    jones[[0, 1, 7, 8, 9, 20, 38, 39], 2:4] = NAN
    jones[5, 3, 1] = complex(1.0, np.inf)  # one float of the second antenna's matrix
    for smooth in (1, 3, 31):
        out, kept, filled, bits, _ = host.InterpolateJonesHost(3, smooth)(jones)
        assert (out.view(np.uint64) == np.tile(value, (40, 3, 1)).view(np.uint64)).all()
        assert kept.tolist() == [40, 31, 40] and filled.tolist() == [0, 9, 0] and not bits.any()
    out, _, _, _, amplitude = host.InterpolateJonesHost(3, 1, True)(np.tile(
        np.eye(2, dtype=np.complex64) * 4, (9, 2, 1)))
    assert (amplitude == 1 * 4).all() and (out == np.tile(np.eye(2), (9, 2, 1))).all()


def test_linear_matrix_is_reproduced_exactly():
    """Elements a + b c with small integer a, b: every step is exact, so a gap is filled with
    the line's own values where t is a dyadic fraction, and held values at the ends."""
    c = np.arange(33)
    line = np.empty((33, 2, 2), np.complex64)
    line[:, 0, 0] = 3 + 2 * c + 1j * (5 - c)
    line[:, 0, 1] = -4 * c + 1j * 7
    line[:, 1, 0] = 16 + 1j * 8 * c
    line[:, 1, 1] = 1 - c - 1j * (2 + 3 * c)
    jones = line.copy()
    jones[9:16] = NAN  # kept 8 and 16: t = k / 8
    jones[17] = NAN  # t = 1 / 2
    jones[:2] = NAN
    jones[31:] = NAN
    out, kept, filled, bits, _ = host.InterpolateJonesHost(7)(jones)
    assert kept[0] == 21 and filled[0] == 12 and bits[0] == 0
    assert (out[2:31] == line[2:31]).all()
    assert (out[:2] == line[2]).all() and (out[31:] == line[30]).all()


@pytest.mark.parametrize("max_gap", [0, 1, 5])
def test_gap_of_max_gap_and_one_more(max_gap):
    jones = np.tile(np.eye(2, dtype=np.complex64), (40, 2, 1))
    jones[10 : 10 + max_gap, 0:2] = NAN  # exactly max_gap (none for 0)
    jones[10 : 11 + max_gap, 2:4] = NAN  # one more
    out, kept, filled, bits, _ = host.InterpolateJonesHost(max_gap)(jones)
    assert kept.tolist() == [40 - max_gap, 39 - max_gap]
    assert filled.tolist() == [max_gap, 0] and bits.tolist() == [0, GAP_LEFT]
    assert np.isfinite(out[:, 0:2]).all()
    assert np.isnan(out[10 : 11 + max_gap, 2:4]).all() and np.isfinite(out[11 + max_gap :]).all()
    # the ends of the band: max_gap channels are held, the next one is not
    jones = np.tile(np.eye(2, dtype=np.complex64), (40, 2, 1))
    jones[:max_gap, 0:2] = NAN
    jones[40 - max_gap :, 0:2] = NAN
    jones[: max_gap + 1, 2:4] = NAN
    jones[39 - max_gap :, 2:4] = NAN
    out, kept, filled, bits, _ = host.InterpolateJonesHost(max_gap)(jones)
    assert filled.tolist() == [2 * max_gap, 2 * max_gap] and bits.tolist() == [0, GAP_LEFT]
    assert np.isnan(out[0, 2:4]).all() and np.isnan(out[39, 2:4]).all()
    assert np.isfinite(out[1:39, 2:4]).all()


def test_fill_status_bits():
    jones = np.tile(np.eye(2, dtype=np.complex64), (12, 4, 1))
    jones[:, 2:4] = NAN  # nothing kept
    jones[3:9, 4:6] = NAN  # a gap that is too long
    jones[:, 6:8] = 0  # kept, but nothing to normalise by
    out, kept, filled, bits, amplitude = host.InterpolateJonesHost(2, normalise=True)(jones)
    assert bits.tolist() == [0, NO_DATA, GAP_LEFT, NO_DATA]
    assert kept.tolist() == [12, 0, 6, 12] and filled.tolist() == [0, 0, 0, 0]
    assert amplitude[0] == 1 and np.isnan(amplitude[1]) and amplitude[2] == 1 and amplitude[3] == 0
    assert np.isnan(out[:, 2:4]).all() and np.isnan(out[:, 6:8]).all()
    status = np.zeros(12, np.uint8)
    status[4] = 0x10
    status[5] = 0x01
    _, kept, filled, _, _ = host.InterpolateJonesHost(2, status_mask=0x0F)(jones, status)
    assert kept.tolist() == [11, 0, 6, 11] and filled.tolist() == [1, 0, 0, 1]


# --------------------------------------------------------------------------------- accuracy
def inverse_bound(y):
    """The largest error of an element of the computed inverse of the float32 matrices `y`
    (..., 2, 2), from the steps, with u = 2^-24, M the largest modulus of an element of the
    matrix and D its determinant. A complex product without fma is within sqrt(5) u < 3 u of
    the true one, relative to the product of the moduli (Brent, Percival & Zimmermann 2007).
    D = a d - b c: two products (3 u M^2 each) and a subtraction per part (u |ad - bc| <=
    2 u M^2): within 8 u M^2. inv = conj(D) / |D|^2 is 1 / D: the error of D enters as
    8 u M^2 / |D| relative, |D|^2 (three operations) and the division add 4 u, and the product
    with an element 3 u more, plus 1 u for the second-order terms: (8 M^2 / |D| + 8) u relative
    to |element| / |D| <= M / |D|."""
    y = y.astype(np.complex128)
    big_m = np.abs(y).max(axis=(-1, -2))
    det = np.abs(y[..., 0, 0] * y[..., 1, 1] - y[..., 0, 1] * y[..., 1, 0])
    return (8 * big_m**2 / det + 8) * 2.0**-24 * big_m / det


def test_corrections_against_a_float64_inverse():
    """`out` with corrections is the inverse of `out` without, element by element within
    inverse_bound, and their product is the identity within 2 M times that (two terms of at
    most M times the error of an element each)."""
    jones, status, model, scale, kinds = gen.make_case(
        2, 120, 6, 4, kinds=("all_kept", "random_holes", "runs", "diagonal", "gap_exact", "ends"))
    scale = np.where(np.isfinite(scale) & (scale != 0), scale, 1).astype(np.complex64)
    for smooth, normalise in ((1, False), (5, True)):
        plain = host.InterpolateJonesHost(4, smooth, normalise, 0x0F)(jones, status, model, scale)
        inverted = host.InterpolateJonesHost(4, smooth, normalise, 0x0F, True)(
            jones, status, model, scale)  # fmt: skip
        for w, g in zip(plain[1:], inverted[1:]):
            assert w is None or (w == g).all()
        y = plain[0].reshape(120, 6, 2, 2)
        c = inverted[0].reshape(120, 6, 2, 2)
        there = np.isfinite(y).all(axis=(2, 3))
        assert there.sum() > 0.8 * there.size
        assert (np.isfinite(c).all(axis=(2, 3)) == there).all()
        y, c = y[there].astype(np.complex128), c[there].astype(np.complex128)
        bound = inverse_bound(y)
        error = np.abs(c - np.linalg.inv(y)).max(axis=(1, 2))
        print(f"smooth {smooth}: inverse off by at most {(error / bound).max():.3f} of the bound")
        assert (error <= bound).all()
        product = np.abs(c @ y - np.eye(2)).max(axis=(1, 2))
        assert (product <= 2 * np.abs(y).max(axis=(1, 2)) * bound).all()


PERIOD = 1024
#: what the four elements of the smooth table are of the bandpass: the diagonal, and leakage
COEFFICIENTS = np.array([[1.0, 0.1 * np.exp(0.7j)], [0.08 * np.exp(-2.1j), 0.9 * np.exp(0.4j)]])


def smooth_case(max_hole, delays=(0.0, 0.0)):
    """(a table of one antenna, f(c) COEFFICIENTS[i][k] exp(2 pi i delays[i] c) as complex64
    with holes of 1 .. max_hole channels, the model of the delays, the truth as complex128)."""
    rs = np.random.RandomState(max_hole)
    c = np.arange(PERIOD)
    rotation = np.exp(2j * np.pi * ((np.asarray(delays)[np.newaxis, :] * c[:, np.newaxis]) % 1.0))
    truth = (gains_gen.bandpass(PERIOD, PERIOD)[:, np.newaxis, np.newaxis] * COEFFICIENTS
             * rotation[:, :, np.newaxis])  # fmt: skip
    jones = truth.astype(np.complex64)
    at = 3
    while at + max_hole < PERIOD - 1:
        length = rs.randint(1, max_hole + 1) if at > 3 else max_hole
        jones[at : at + length] = NAN
        at += length + rs.randint(1, 5)
    return jones, rotation.astype(np.complex64), truth


def accuracy_bound(max_hole):
    """Per element, DESIGN.md section 22's bound for the element's own f = COEFFICIENTS[i][k]
    bandpass: linear interpolation between samples h = max_hole + 1 apart is off by at most
    h^2 / 8 max|f''|, and the float32 steps (the rounding of the samples and of the model, two
    rotations and the interpolation) are given 8 units of 2^-23 max|f|. (2, 2)."""
    curvature = gains_gen.bandpass_curvature(PERIOD)
    largest = np.abs(gains_gen.bandpass(PERIOD, PERIOD)).max()
    return np.abs(COEFFICIENTS) * ((max_hole + 1) ** 2 / 8 * curvature + 8 * 2.0**-23 * largest)


@pytest.mark.parametrize("max_hole", [1, 4, 16, 64])
def test_accuracy_on_a_smooth_bandpass(max_hole):
    jones, _, truth = smooth_case(max_hole)
    out, kept, filled, bits, _ = host.InterpolateJonesHost(max_hole)(jones)
    assert bits[0] == 0 and filled[0] > PERIOD // 4 and kept[0] + filled[0] == PERIOD
    error = np.abs(out.astype(np.complex128) - truth).max(axis=0)
    bound = accuracy_bound(max_hole)
    print(f"holes of up to {max_hole}: error / bound {(error / bound).round(3).tolist()}")
    assert (error <= bound).all()


@pytest.mark.parametrize("max_hole", [1, 4, 16, 64])
def test_the_model_is_what_makes_a_delay_harmless(max_hole):
    """The same table under delays of 0.2 and -0.13 turns per channel on its two rows: with the
    per-row model every element meets the same bound; without it the wound phase misses the
    bound by more than a factor of 100 in every element."""
    jones, model, truth = smooth_case(max_hole, (0.2, -0.13))
    fn = host.InterpolateJonesHost(max_hole)
    out, _, filled, bits, _ = fn(jones, model=model)
    assert bits[0] == 0 and filled[0] > PERIOD // 4
    error = np.abs(out.astype(np.complex128) - truth).max(axis=0)
    plain = np.abs(fn(jones)[0].astype(np.complex128) - truth).max(axis=0)
    bound = accuracy_bound(max_hole)
    print(f"holes of up to {max_hole}: error / bound {(error / bound).round(3).tolist()} with "
          f"the model, {(plain / bound).round(1).tolist()} without")  # fmt: skip
    assert (error <= bound).all()
    assert (plain > 100 * bound).all()


# ---------------------------------------------------------------------------- the diagonal
def test_jones_diagonal_host():
    jones = gen.make_case(4, 7, 3, 2)[0]
    jones[2, 3, 1] = complex(-0.0, np.nan)
    gains = host.JonesDiagonalHost()(jones)
    assert gains.shape == (7, 6) and gains.dtype == np.complex64
    for p in range(6):
        assert (gains[:, p].view(np.uint64) == jones[:, p, p % 2].copy().view(np.uint64)).all()
    assert host.JonesDiagonalHost()(jones[:1, :1]).shape == (1, 1)
    for bad in (jones.astype(np.complex128), jones[0], jones[:0], jones[:, :0], jones[:, :, :1],
                jones.real):  # fmt: skip
        with pytest.raises(ValueError, match="jones"):
            host.JonesDiagonalHost()(bad)


# ----------------------------------------------------------------------------------- errors
def test_host_errors():
    assert issubclass(host.InterpolateJonesHost, host.InterpolateGainsHost)
    for bad in (-1, 16385):
        with pytest.raises(ValueError, match="max_gap"):
            host.InterpolateJonesHost(bad)
    for bad in (1.0, True, "3", None):
        with pytest.raises(TypeError, match="max_gap"):
            host.InterpolateJonesHost(bad)
    for bad in (0, 2, 4, 30, 33, -1):
        with pytest.raises(ValueError, match="smooth"):
            host.InterpolateJonesHost(1, bad)
    for bad in (3.0, False):
        with pytest.raises(TypeError, match="smooth"):
            host.InterpolateJonesHost(1, bad)
    for bad in (-1, 256):
        with pytest.raises(ValueError, match="status_mask"):
            host.InterpolateJonesHost(1, status_mask=bad)
    with pytest.raises(TypeError, match="status_mask"):
        host.InterpolateJonesHost(1, status_mask=1.0)
    fn = host.InterpolateJonesHost(np.int64(16384), np.int32(31))
    assert (fn.max_gap, fn.smooth, fn.normalise, fn.status_mask, fn.corrections) == (
        16384, 31, False, 255, False)  # fmt: skip
    fn = host.InterpolateJonesHost(0, 1, 1, 0, 1)
    assert (fn.max_gap, fn.normalise, fn.status_mask, fn.corrections) == (0, True, 0, True)
    cls = host.InterpolateJonesHost
    assert (cls.MAX_CHANNELS, cls.MAX_GAP, cls.MAX_SMOOTH, cls.MAX_INPUTS, cls.NO_DATA,
            cls.GAP_LEFT) == (16384, 16384, 31, 2048, 1, 2)  # fmt: skip
    good, status, model, scale, _ = gen.make_case(1, 6, 2, 2)
    fn(good, status, model, scale)
    for bad in (good.astype(np.complex128), good[0], good[:0], good[:, :0], good[:, :3],
                good[:, :, :1], good[:, :, 0], good.real, np.zeros((16385, 2, 2), np.complex64),
                np.zeros((1, 2050, 2), np.complex64)):  # fmt: skip
        with pytest.raises(ValueError, match="jones"):
            fn(bad, status, model, scale)
    for bad in (status.astype(np.int8), status[:5], status[:, np.newaxis], np.zeros(7, np.uint8)):
        with pytest.raises(ValueError, match="status"):
            fn(good, bad)
    for bad in (model.astype(np.complex128), model[:5], model[:, :2], model[:, 0], model.real,
                good):  # fmt: skip
        with pytest.raises(ValueError, match="model"):
            fn(good, model=bad)
    for bad in (scale.astype(np.complex128), scale[:2], scale[:, np.newaxis], scale.real):
        with pytest.raises(ValueError, match="scale"):
            fn(good, scale=bad)
    fn(np.zeros((16384, 2, 2), np.complex64))
    fn(np.zeros((1, 2048, 2), np.complex64))
    for bad in ((0, 2), (16385, 2), (4, 0), (4, 3), (4, 2050)):
        with pytest.raises(ValueError):
            fn.check_shape(*bad)
    fn.check_shape(16384, 2048)


def test_template_and_operation_errors(context, queue):
    with pytest.raises(ValueError):
        ingest.InterpolateJonesTemplate(context, 8, tuning={"wgs": 256})
    assert ingest.InterpolateJonesTemplate(context, 8, tuning={}).tuning == {}
    assert ingest.InterpolateJonesTemplate.autotune(context) == {}
    assert ingest.InterpolateJonesTemplate.TUNING_KEYS == ()
    assert ingest.InterpolateJonesTemplate.host_class is host.InterpolateJonesHost
    assert ingest.InterpolateJonesTemplate.KERNEL == "ksp_interpolate_jones"
    assert ingest.InterpolateJonesTemplate.operation_class is ingest.InterpolateJones
    for name, bads in (("max_gap", (-1, 16385)), ("smooth", (0, 2, 33)), ("status_mask", (-1, 256))):
        for bad in bads:
            with pytest.raises(ValueError, match=name):
                ingest.InterpolateJonesTemplate(context, **{"max_gap": 8, name: bad})
    for name in ("max_gap", "smooth", "status_mask"):
        with pytest.raises(TypeError, match=name):
            ingest.InterpolateJonesTemplate(context, **{"max_gap": 8, name: 1.5})
    template = ingest.InterpolateJonesTemplate(context, 8)
    assert template.kernel.name == "ksp_interpolate_jones"
    assert (template.max_gap, template.smooth, template.normalise, template.status,
            template.status_mask, template.model, template.scale, template.corrections) == (
        8, 1, False, True, 255, True, False, False)  # fmt: skip
    for args in [(0, 4), (-1, 4), (16385, 4), (4, 0), (4, -2), (4, 3), (4, 2050)]:
        with pytest.raises(ValueError):
            template.instantiate(queue, *args)
    assert isinstance(template.instantiate(queue, 16384, 2), ingest.InterpolateJones)
    assert isinstance(template.instantiate(queue, 1, 2048), ingest.InterpolateJones)
    fn = ingest.InterpolateJonesTemplate(context, 5, 9, True, False, 0x30, False, True,
                                         True).instantiate(queue, 100, 8)  # fmt: skip
    assert fn.parameters() == {"max_gap": 5, "smooth": 9, "normalise": True, "status": False,
                               "status_mask": 0x30, "model": False, "scale": True,
                               "corrections": True, "channels": 100, "n_inputs": 8}  # fmt: skip
    # the diagonal
    with pytest.raises(ValueError):
        ingest.JonesDiagonalTemplate(context, tuning={"wgs": 256})
    template = ingest.JonesDiagonalTemplate(context)
    assert template.tuning == {} and ingest.JonesDiagonalTemplate.autotune(context) == {}
    assert template.kernel.name == ingest.JonesDiagonalTemplate.KERNEL == "ksp_jones_diagonal"
    assert ingest.JonesDiagonalTemplate.host_class is host.JonesDiagonalHost
    assert ingest.JonesDiagonalTemplate.operation_class is ingest.JonesDiagonal
    for args, name in [((0, 4), "channels"), ((-1, 4), "channels"), ((4, 0), "n_inputs")]:
        with pytest.raises(ValueError, match=name):
            template.instantiate(queue, *args)
    assert template.instantiate(queue, 3, 5).parameters() == {"channels": 3, "n_inputs": 5}


def test_host_from_device(context, queue):
    jones, status, model, scale, _ = gen.make_case(1, 10, 3, 2)
    for with_status, with_model, with_scale, normalise, corrections in VARIANTS:
        template = ingest.InterpolateJonesTemplate(context, 2, 3, normalise, with_status, 0xFF,
                                                   with_model, with_scale, corrections)  # fmt: skip
        adapter = ingest.InterpolateJonesHostFromDevice(template, queue)
        del queue.launches[:]
        given = dict(status=status if with_status else None, model=model if with_model else None,
                     scale=scale if with_scale else None)  # fmt: skip
        out = adapter(jones, **given)
        assert len(out) == 5 and (out[4] is not None) == normalise
        for o, shape, dtype in zip(out, [(10, 6, 2)] + [(3,)] * 4,
                                   (np.complex64, np.int32, np.int32, np.uint8, f32)):  # fmt: skip
            assert o is None or (o.shape, o.dtype) == (shape, dtype)
        assert [name for name, _ in queue.launches] == ["ksp_interpolate_jones"]
        assert [int(a) for a in queue.launches[0][1][9:11]] == [10, 6]
        for name, present in (("status", with_status), ("model", with_model), ("scale", with_scale)):
            wrong = dict(given)
            wrong[name] = None if present else {"status": status, "model": model, "scale": scale}[name]
            with pytest.raises(TypeError, match=name):
                adapter(jones, **wrong)
    adapter = ingest.InterpolateJonesHostFromDevice(
        ingest.InterpolateJonesTemplate(context, 2, status=False, model=False), queue)
    with pytest.raises(ValueError):
        adapter(jones[:0])
    with pytest.raises(ValueError):
        adapter(jones[:, :3])
    del queue.launches[:]
    gains = ingest.JonesDiagonalHostFromDevice(ingest.JonesDiagonalTemplate(context), queue)(jones)
    assert (gains.shape, gains.dtype) == ((10, 6), np.complex64)
    assert [name for name, _ in queue.launches] == ["ksp_jones_diagonal"]
    with pytest.raises(ValueError):
        ingest.JonesDiagonalHostFromDevice(ingest.JonesDiagonalTemplate(context), queue)(jones[:0])


# ----------------------------------------------------------------------------------- wiring
@pytest.mark.parametrize("with_status, with_model, with_scale, normalise, corrections", VARIANTS)
def test_slots_and_launch_arguments(with_status, with_model, with_scale, normalise, corrections,
                                    context, queue):  # fmt: skip
    template = ingest.InterpolateJonesTemplate(context, 11, 5, normalise, with_status, 0x3C,
                                               with_model, with_scale, corrections)  # fmt: skip
    fn = template.instantiate(queue, 300, 58)
    names = (["jones"] + (["status"] if with_status else []) + (["model"] if with_model else [])
             + (["scale"] if with_scale else []) + ["out", "kept", "filled", "fill_status"]
             + (["mean_amplitude"] if normalise else []))  # fmt: skip
    assert list(fn.slots) == names
    shapes = {"jones": ((300, 58, 2), np.complex64), "status": ((300,), np.uint8),
              "model": ((300, 58), np.complex64), "scale": ((58,), np.complex64),
              "out": ((300, 58, 2), np.complex64), "kept": ((29,), np.int32),
              "filled": ((29,), np.int32), "fill_status": ((29,), np.uint8),
              "mean_amplitude": ((29,), f32)}  # fmt: skip
    for name, slot in fn.slots.items():
        assert (slot.shape, slot.dtype) == shapes[name], name
    # a dimension object of its own for everything that can be padded; the last axis of the
    # tables cannot
    dims = [d for slot in fn.slots.values() for d in slot.dimensions]
    assert len({id(d) for d in dims}) == len(dims) == len(fn.slots) + 4 + with_model
    for name in ("jones", "out"):
        assert fn.slots[name].dimensions[2].exact
    accel.Dimension(58, min_padded_size=100).link(fn.slots["jones"].dimensions[1])
    accel.Dimension(58, min_padded_size=150).link(fn.slots["out"].dimensions[1])
    if with_model:
        accel.Dimension(58, min_padded_size=200).link(fn.slots["model"].dimensions[1])
    fn()
    assert [name for name, _ in queue.launches] == ["ksp_interpolate_jones"]
    args = queue.launches[0][1]
    assert len(args) == 18
    order = ["jones", "status", "model", "scale", "out", "kept", "filled", "fill_status",
             "mean_amplitude"]  # fmt: skip
    for got, name in zip(args[:9], order):
        assert got is (fn.buffer(name).buffer if name in names else None), name
    assert all(isinstance(a, np.int32) for a in args[9:])
    assert [int(a) for a in args[9:11]] == [300, 58]
    assert fn.buffer("jones").padded_shape[2] == fn.buffer("out").padded_shape[2] == 2
    assert int(args[11]) == fn.buffer("jones").padded_shape[1] >= 100
    assert int(args[12]) == (fn.buffer("model").padded_shape[1] if with_model else 0)
    assert int(args[12]) == (208 if with_model else 0)
    assert int(args[13]) == fn.buffer("out").padded_shape[1] >= 150
    assert int(args[11]) != int(args[13])
    assert [int(a) for a in args[14:]] == [11, 5, 0x3C, int(corrections)]


def test_in_place_binding(context, queue):
    """out bound to the buffer of jones: the launcher gets the same pointer and stride twice."""
    fn = ingest.InterpolateJonesTemplate(context, 4, status=False, model=False).instantiate(
        queue, 20, 6)  # fmt: skip
    fn.ensure_all_bound()
    fn.bind(out=fn.buffer("jones"))
    fn()
    args = queue.launches[0][1]
    assert args[0] is args[4] is fn.buffer("jones").buffer and int(args[11]) == int(args[13])


def test_jones_diagonal_slots_and_launch_arguments(context, queue):
    fn = ingest.JonesDiagonalTemplate(context).instantiate(queue, 300, 58)
    assert list(fn.slots) == ["jones", "gains"]
    assert (fn.slots["jones"].shape, fn.slots["jones"].dtype) == ((300, 58, 2), np.complex64)
    assert (fn.slots["gains"].shape, fn.slots["gains"].dtype) == ((300, 58), np.complex64)
    dims = [d for slot in fn.slots.values() for d in slot.dimensions]
    assert len({id(d) for d in dims}) == len(dims) == 5 and fn.slots["jones"].dimensions[2].exact
    accel.Dimension(58, min_padded_size=100).link(fn.slots["jones"].dimensions[1])
    accel.Dimension(58, min_padded_size=150).link(fn.slots["gains"].dimensions[1])
    fn()
    assert [name for name, _ in queue.launches] == ["ksp_jones_diagonal"]
    args = queue.launches[0][1]
    assert len(args) == 6 and all(isinstance(a, np.int32) for a in args[2:])
    assert args[0] is fn.buffer("jones").buffer and args[1] is fn.buffer("gains").buffer
    assert [int(a) for a in args[2:]] == [300, 58, fn.buffer("jones").padded_shape[1],
                                          fn.buffer("gains").padded_shape[1]]  # fmt: skip
    assert int(args[4]) >= 100 and int(args[5]) >= 150 and int(args[4]) != int(args[5])


def test_between_solve_jones_and_apply_jones(context, queue):
    """solve_jones -> jones_diagonal -> fit_delays -> interpolate_jones -> apply_jones: the
    diagonal feeds the fit, the new step reads the solver's table and status and the fit's
    model, and apply_jones multiplies by its out; every shared array has one padded size."""
    rows, n_inputs = 64, 12
    baselines, n_quads = n_inputs * (n_inputs + 1) // 2, 21
    solve = ingest.SolveJonesTemplate(context).instantiate(queue, rows, baselines, n_inputs)
    diagonal = ingest.JonesDiagonalTemplate(context).instantiate(queue, rows, n_inputs)
    fit = ingest.FitDelaysTemplate(context, 1e6).instantiate(queue, rows, n_inputs)
    interp = ingest.InterpolateJonesTemplate(context, 8, corrections=True).instantiate(
        queue, rows, n_inputs)  # fmt: skip
    apply_jones = ingest.ApplyJonesTemplate(context).instantiate(
        queue, rows, baselines, n_inputs, n_quads)  # fmt: skip
    accel.Dimension(n_inputs, min_padded_size=40).link(solve.slots["jones"].dimensions[1])
    accel.Dimension(n_inputs, min_padded_size=70).link(apply_jones.slots["jones"].dimensions[1])
    accel.Dimension(n_inputs, min_padded_size=90).link(fit.slots["model"].dimensions[1])
    accel.Dimension(n_inputs, min_padded_size=50).link(fit.slots["gains"].dimensions[1])
    seq = accel.OperationSequence(
        queue, [("solve", solve), ("diagonal", diagonal), ("fit", fit), ("interp", interp),
                ("apply", apply_jones)],
        compounds={"jones": ["solve:jones", "diagonal:jones", "interp:jones"],
                   "status": ["solve:status", "fit:status", "interp:status"],
                   "gains": ["diagonal:gains", "fit:gains"],
                   "k": ["fit:model", "interp:model"],
                   "corr": ["interp:out", "apply:jones"]})  # fmt: skip
    assert {"jones", "status", "gains", "k", "corr", "interp:kept", "interp:filled",
            "interp:fill_status"} <= set(seq.slots)  # fmt: skip
    seq()
    assert [name for name, _ in queue.launches] == [
        "ksp_solve_jones", "ksp_jones_diagonal", "ksp_fit_delays", "ksp_interpolate_jones",
        "ksp_apply_jones"]  # fmt: skip
    solve_args, diag_args, fit_args, interp_args, apply_args = (l[1] for l in queue.launches)
    assert solve_args[5] is diag_args[0] is interp_args[0] is seq.buffer("jones").buffer
    assert solve_args[7] is fit_args[1] is interp_args[1] is seq.buffer("status").buffer
    assert diag_args[1] is fit_args[0] is seq.buffer("gains").buffer
    assert fit_args[6] is interp_args[2] is seq.buffer("k").buffer
    assert interp_args[4] is seq.buffer("corr").buffer
    assert any(a is seq.buffer("corr").buffer for a in apply_args)
    jones_stride = seq.buffer("jones").padded_shape[1]
    assert int(solve_args[16]) == int(diag_args[4]) == int(interp_args[11]) == jones_stride >= 40
    assert int(diag_args[5]) == int(fit_args[9]) == seq.buffer("gains").padded_shape[1] >= 50
    assert int(interp_args[12]) == int(fit_args[10]) == seq.buffer("k").padded_shape[1] == 96
    assert int(interp_args[13]) == seq.buffer("corr").padded_shape[1] >= 70
    assert seq.buffer("jones").padded_shape[2] == seq.buffer("corr").padded_shape[2] == 2
    assert [int(a) for a in interp_args[9:11]] == [rows, n_inputs]
    assert [int(a) for a in interp_args[14:]] == [8, 1, 255, 1]


def test_host_chain_meets_its_conditions():
    """The scan of the chain test on the host classes alone: every gap of the calibrator is
    filled, no target sample carries flag_value, every sample of the 40 channels does when the
    solver's own corrections are applied directly, and the calibrated target is the identity
    coherency times the flux to within CHAIN_MEASURED (asserted at twice the measurement)."""
    scan = gen.chain_scan()
    out = gen.chain_host(scan)
    flagged, n_ant = scan["flagged"], gen.CHAIN["n_inputs"] // 2
    assert flagged.sum() == 40 and scan["baselines"] == 36
    assert np.isnan(out["jones"][flagged]).all() and np.isfinite(out["jones"][~flagged]).all()
    assert not out["fit:fit_status"].any() and not out["interp:fill_status"].any()
    assert (out["fit:delays"][:2] == 0).all() and (out["fit:phasors"][:2] == 1).all()
    assert (out["interp:kept"] == 216).all() and (out["interp:filled"] == 40).all()
    assert len(out["interp:kept"]) == n_ant and np.isfinite(out["corr"]).all()
    assert not out["apply:out_flags"].any() and (out["apply:out_weights"] > 0).all()
    distance = gen.chain_distance(scan, out["apply:out_vis"])
    print(f"chain: calibrated target within {distance:.5f} of the identity coherency")
    assert 0.9 * gen.CHAIN_MEASURED <= distance <= 2 * gen.CHAIN_MEASURED
    direct = host.SolveJonesHost(gen.CHAIN["max_iterations"], corrections=True)(
        scan["cal_vis"], scan["pairs"], scan["weights"], scan["cal_flags"])[0]  # fmt: skip
    lost = host.ApplyJonesHost(gen.CHAIN["flag_value"])(
        scan["target_vis"], direct, scan["quad_antennas"], scan["quads"], scan["weights"],
        scan["target_flags"])[2]  # fmt: skip
    assert (lost[flagged] == gen.CHAIN["flag_value"]).all() and not lost[~flagged].any()


# ------------------------------------------------------------------- the launchers' checks
@pytest.fixture(scope="module")
def lib():
    from katsdpsigproc_amd import _lib, build_native

    if not os.path.exists(_lib.LIB_PATH):
        build_native.build()
    return _lib.load()


POINTERS = ["jones", "status", "model", "scale", "out", "kept", "filled", "fill_status",
            "mean_amplitude"]  # fmt: skip
NUMBERS = ["channels", "n_inputs", "jones_stride", "model_stride", "out_stride", "max_gap",
           "smooth", "status_mask", "corrections"]  # fmt: skip


def test_argument_validation_without_gpu(lib):
    from katsdpsigproc_amd import _lib

    # never dereferenced: every call below fails its checks first. Nine arrays far apart.
    p = {name: ctypes.c_void_p((i + 1) << 32) for i, name in enumerate(POINTERS)}
    good = dict(channels=4, n_inputs=8, jones_stride=8, model_stride=8, out_stride=8, max_gap=2,
                smooth=3, status_mask=255, corrections=0)  # fmt: skip

    def call(device=0, **changed):
        a = dict(p, **good)
        a.update(changed)
        rc = lib.ksp_interpolate_jones(device, None, *(a[name] for name in POINTERS),
                                       *(a[name] for name in NUMBERS))  # fmt: skip
        assert rc != 0
        return _lib.last_error()

    for name in ("jones", "out", "kept", "filled", "fill_status"):
        assert f"invalid argument: {name} is NULL" in call(**{name: None})
    for bad in (0, -1, 16385):
        assert "invalid argument: channels must be 1..16384" in call(channels=bad)
    for bad in (0, -2, 1, 7, 2050, 2049):
        assert "invalid argument: n_inputs must be even and 2..2048" in call(
            n_inputs=bad, jones_stride=4096, model_stride=4096, out_stride=4096)
    for bad in (-1, 16385):
        assert "invalid argument: max_gap must be 0..16384" in call(max_gap=bad)
    for bad in (0, -1, 2, 30, 32, 33):
        assert "invalid argument: smooth must be odd and 1..31" in call(smooth=bad)
    for bad in (-1, 256):
        assert "invalid argument: status_mask must be 0..255" in call(status_mask=bad)
    for bad in (-1, 2):
        assert "invalid argument: corrections must be 0 or 1" in call(corrections=bad)
    for name in ("jones", "model", "out"):
        assert f"invalid argument: {name}_stride is smaller than n_inputs" in call(
            **{name + "_stride": 7})
    # the order of the checks: everything wrong at once, then one thing fewer at a time
    wrong = dict(channels=0, n_inputs=0, jones_stride=-1, model_stride=-1, out_stride=-1,
                 max_gap=-1, smooth=2, status_mask=-1, corrections=2)  # fmt: skip
    nulls = dict.fromkeys(p)
    for name in ("jones", "out", "kept", "filled", "fill_status"):
        assert f"invalid argument: {name} is NULL" in call(**nulls, **wrong)
        nulls[name] = p[name]
    order = [("channels", "channels must be"), ("n_inputs", "n_inputs must be"),
             ("max_gap", "max_gap must be"), ("smooth", "smooth must be"),
             ("status_mask", "status_mask must be"), ("corrections", "corrections must be"),
             ("jones_stride", "jones_stride is smaller"), ("model_stride", "model_stride is smaller"),
             ("out_stride", "out_stride is smaller")]  # fmt: skip
    overlapping = dict(out=ctypes.c_void_p(p["jones"].value + 8), model=p["jones"])
    for name, message in order:
        assert message in call(**wrong, **overlapping), name
        wrong[name] = good[name]
    assert "out overlaps jones" in call(**overlapping)
    # an absent array's stride is not looked at, and every optional array may be absent
    assert "hipSetDevice(device) failed" in call(device=-1, model=None, model_stride=-1)
    assert "hipSetDevice(device) failed" in call(device=-1, status=None, scale=None,
                                                 mean_amplitude=None)  # fmt: skip

    def at(name, offset):
        return ctypes.c_void_p(p[name].value + offset)

    # the bytes from the first element to the last: rows of two complex64 in jones and out,
    # single complex64 in model
    extent, model_extent = (3 * 8 + 8) * 16, (3 * 8 + 8) * 8
    message = "invalid argument: out overlaps jones without being jones with the same stride"
    assert message in call(out=at("jones", extent - 1))
    assert message in call(out=at("jones", -(extent - 1)))
    assert message in call(out=p["jones"], out_stride=9)
    assert message in call(out=at("jones", 8))
    assert "invalid argument: out overlaps model" in call(out=p["model"])
    assert "invalid argument: out overlaps model" in call(out=at("model", model_extent - 1))
    assert "invalid argument: out overlaps model" in call(out=at("model", -(extent - 1)))
    assert "invalid argument: out overlaps model" in call(out=p["jones"], model=p["jones"])
    # in place, arrays that only touch and the limits pass every check: what is left to fail is
    # the first device call, which device -1 fails on any machine
    for passing in (dict(out=p["jones"]), dict(out=at("jones", extent)), dict(out=at("jones", -extent)),
                    dict(out=at("model", model_extent)), dict(out=at("model", -extent)),
                    dict(out=p["model"], model=None), dict(channels=16384, max_gap=16384, smooth=31),
                    dict(n_inputs=2048, jones_stride=2048, model_stride=2048, out_stride=2048),
                    dict(channels=1, n_inputs=2, max_gap=0, smooth=1, status_mask=0, corrections=1)):  # fmt: skip
        assert "hipSetDevice(device) failed" in call(device=-1, **passing)


def test_jones_diagonal_argument_validation_without_gpu(lib):
    from katsdpsigproc_amd import _lib

    jones, gains = ctypes.c_void_p(1 << 32), ctypes.c_void_p(2 << 32)
    good = dict(jones=jones, gains=gains, channels=4, n_inputs=5, jones_stride=5, gains_stride=5)

    def call(device=0, **changed):
        a = dict(good, **changed)
        rc = lib.ksp_jones_diagonal(device, None, *a.values())
        assert rc != 0
        return _lib.last_error()

    assert list(good) == ["jones", "gains", "channels", "n_inputs", "jones_stride", "gains_stride"]
    for name in ("jones", "gains"):
        assert f"invalid argument: {name} is NULL" in call(**{name: None})
    for bad in (0, -1):
        assert "invalid argument: channels must be at least 1" in call(channels=bad)
        assert "invalid argument: n_inputs must be at least 1" in call(n_inputs=bad)
    for name in ("jones", "gains"):
        assert f"invalid argument: {name}_stride is smaller than n_inputs" in call(
            **{name + "_stride": 4})
    wrong = dict(channels=0, n_inputs=0, jones_stride=-1, gains_stride=-1)
    assert "jones is NULL" in call(jones=None, gains=None, **wrong)
    assert "gains is NULL" in call(gains=None, **wrong)
    for name, message in (("channels", "channels must be"), ("n_inputs", "n_inputs must be"),
                          ("jones_stride", "jones_stride is smaller"),
                          ("gains_stride", "gains_stride is smaller")):  # fmt: skip
        assert message in call(gains=jones, **wrong), name
        wrong[name] = good[name]
    assert "invalid argument: gains overlaps jones" in call(gains=jones)
    extent = (3 * 5 + 5) * 16  # of jones; gains is half as long
    assert "gains overlaps jones" in call(gains=ctypes.c_void_p(jones.value + extent - 1))
    assert "gains overlaps jones" in call(gains=ctypes.c_void_p(jones.value - extent // 2 + 1))
    assert "array too large for one launch" in call(
        gains=ctypes.c_void_p(1 << 50), channels=2**31 - 1, n_inputs=2**10, jones_stride=2**10,
        gains_stride=2**10)  # fmt: skip
    for passing in (dict(gains=ctypes.c_void_p(jones.value + extent)),
                    dict(gains=ctypes.c_void_p(jones.value - extent // 2)),
                    dict(channels=1, n_inputs=1, jones_stride=1, gains_stride=1)):  # fmt: skip
        assert "hipSetDevice(device) failed" in call(device=-1, **passing)


def test_header_binding_and_exports(lib):
    from katsdpsigproc_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "katsdpsigproc_hip.h")).read()
    comment = re.search(r"/\* interpolate_jones:.*?\*/", text, re.S).group(0)
    assert "InterpolateJonesHost" in comment
    assert re.search(r"/\* jones_diagonal:.*?\*/", text, re.S) is not None
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for symbol, names in (("ksp_interpolate_jones", POINTERS + NUMBERS),
                          ("ksp_jones_diagonal", ["jones", "gains", "channels", "n_inputs",
                                                  "jones_stride", "gains_stride"])):  # fmt: skip
        declaration = re.search(r"int %s\((.*?)\);" % symbol, text, re.S)
        assert declaration is not None
        parameters = [" ".join(part.split()) for part in declaration.group(1).split(",")]
        argtypes = _lib.SIGNATURES[symbol]
        assert len(parameters) == len(argtypes) == len(names) + 2
        for parameter, argtype in zip(parameters, argtypes):
            assert ("*" in parameter) == (argtype is ctypes.c_void_p), parameter
            assert argtype in (ctypes.c_int, ctypes.c_void_p)
        found = [parameter.replace("*", " ").split()[-1] for parameter in parameters]
        assert found == ["device", "stream"] + names
        assert hasattr(lib, symbol)
        assert symbol in _lib.declared_symbols()
    assert lib.ksp_abi_version() == _lib.ABI_VERSION == 5
    for name in ("InterpolateJonesTemplate", "InterpolateJones", "InterpolateJonesHostFromDevice",
                 "JonesDiagonalTemplate", "JonesDiagonal", "JonesDiagonalHostFromDevice"):  # fmt: skip
        assert hasattr(ingest, name)
    assert hasattr(host, "InterpolateJonesHost") and hasattr(host, "JonesDiagonalHost")
