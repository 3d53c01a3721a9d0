"""Filling solved gains across flagged channels without a GPU:
``rfi.host.InterpolateGainsHost`` against a loop of float32 scalars, the identity on kept
channels, known answers, gap handling at ``max_gap`` and ``max_gap + 1``, the accuracy bound of
linear interpolation on a smooth bandpass with and without the delay model; argument errors,
slot lists and every launch argument of every variant on the fake backend, the sequence
solve_gains -> fit_delays -> interpolate_gains -> apply_gains, and the argument checks of
``ksp_interpolate_gains``, which come before any device call."""

import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from katsdpsigproc_amd import accel
from katsdpsigproc_amd.rfi import host, ingest
from tests import inputs_interpolate_gains as gen
from tests.fakes import FakeContext
from tests.inputs_interpolate_gains import assert_same

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


def scalar_product(a, b):
    return (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])


def scalar_column(g, status, m, scale, max_gap, smooth, normalise, mask, corrections):
    """One input: lists of (float32, float32) `g` and `m` (or None), `status` a list of ints
    (or None), `scale` a pair (or None). Returns (out as a list of pairs, kept, filled,
    fill_status, mean_amplitude or None)."""
    channels = len(g)
    nan = f32(np.nan)
    kept, s = [], []
    for c in range(channels):
        ok = bool(np.isfinite(g[c][0]) and np.isfinite(g[c][1]))
        if status is not None:
            ok = ok and (status[c] & mask) == 0
        if m is not None:
            ok = ok and bool(np.isfinite(m[c][0]) and np.isfinite(m[c][1]))
            s.append((g[c][0] * m[c][0] + g[c][1] * m[c][1], g[c][1] * m[c][0] - g[c][0] * m[c][1]))
        else:
            s.append(g[c])
        kept.append(ok)
    n_kept = sum(kept)
    failed = n_kept == 0
    if smooth > 1:
        reach = smooth // 2
        smoothed = list(s)
        for c in range(channels):
            if not kept[c]:
                continue
            re, im, n = f32(0), f32(0), 0
            for j in range(max(0, c - reach), min(channels - 1, c + reach) + 1):
                if kept[j]:
                    re, im, n = re + s[j][0], im + s[j][1], n + 1
            smoothed[c] = (re / f32(n), im / f32(n))
        s = smoothed
    mean_amplitude = None
    if normalise:
        c_pad = 1
        while c_pad < channels:
            c_pad *= 2
        terms = [f32(0)] * c_pad
        for c in range(channels):
            if kept[c]:
                terms[c] = np.sqrt(s[c][0] * s[c][0] + s[c][1] * s[c][1])
        mean_amplitude = scalar_tree(terms) / f32(n_kept) if n_kept else nan
        if mean_amplitude > 0 and mean_amplitude < np.inf:
            s = [(x[0] / mean_amplitude, x[1] / mean_amplitude) for x in s]
        else:
            failed = True
    out, filled, gap_left = [], 0, False
    for c in range(channels):
        if failed:
            out.append((nan, nan))
            continue
        if kept[c]:
            y = s[c]
        else:
            below = [j for j in range(c) if kept[j]]
            above = [j for j in range(c + 1, channels) if kept[j]]
            y = None
            if below and above:
                l, r = below[-1], above[0]
                if r - l - 1 <= max_gap:
                    t = f32(c - l) / f32(r - l)
                    y = tuple(s[l][i] + (s[r][i] - s[l][i]) * t for i in range(2))
            elif below:
                if c - below[-1] <= max_gap:
                    y = s[below[-1]]
            elif above[0] - c <= max_gap:
                y = s[above[0]]
            if y is None:
                y = (nan, nan)
                gap_left = True
            else:
                filled += 1
        if m is not None:
            y = scalar_product(y, m[c])
        if scale is not None:
            y = scalar_product(y, scale)
        if corrections:
            q = y[0] * y[0] + y[1] * y[1]
            y = (y[0] / q, -y[1] / q) if q > 0 else (nan, nan)
        assert all(type(part) is f32 for part in y)
        out.append(y)
    bits = NO_DATA if failed else GAP_LEFT if gap_left else 0
    return out, n_kept, filled, bits, mean_amplitude


def scalar_loop(gains, status, model, scale, max_gap, smooth, normalise, mask, corrections):
    def pairs(column):
        return [(f32(v.real), f32(v.imag)) for v in column]

    channels, n_inputs = gains.shape
    out = np.empty((channels, n_inputs), np.complex64)
    kept, filled = np.empty(n_inputs, np.int32), np.empty(n_inputs, np.int32)
    fill_status = np.empty(n_inputs, np.uint8)
    mean_amplitude = np.empty(n_inputs, f32) if normalise else None
    with np.errstate(all="ignore"):
        for p in range(n_inputs):
            column, kept[p], filled[p], fill_status[p], a = scalar_column(
                pairs(gains[:, p]), None if status is None else [int(v) for v in status],
                None if model is None else pairs(model[:, p]),
                None if scale is None else pairs(scale[p : p + 1])[0],
                max_gap, smooth, normalise, mask, corrections)  # fmt: skip
            out.real[:, p] = [y[0] for y in column]
            out.imag[:, p] = [y[1] for y in column]
            if normalise:
                mean_amplitude[p] = a
    return out, kept, filled, fill_status, mean_amplitude


def check(want, got, what=""):
    assert len(want) == len(got) == 5
    for name, w, g in zip(OUTPUTS, want, got):
        if w is None:
            assert g is None, name
        else:
            assert_same(w, g, f"{name} {what}")


@pytest.mark.parametrize("channels, max_gap, smooth, variant", [
    (1, 1, 1, (True, True, True, True, True)), (2, 0, 3, (False, True, False, True, False)),
    (3, 2, 1, (True, False, True, False, True)), (37, 3, 5, (True, True, True, True, True)),
    (64, 4, 31, (False, False, False, True, False)), (65, 1, 1, (False, False, False, False, False)),
    (130, 8, 9, (True, True, False, False, True)), (100, 16384, 3, (False, True, True, True, False)),
])  # fmt: skip
def test_host_against_scalar_loop(channels, max_gap, smooth, variant):
    with_status, with_model, with_scale, normalise, corrections = variant
    n_inputs = len(gen.KINDS) + 3
    gains, status, model, scale, _ = gen.make_case(channels + smooth, channels, n_inputs, max_gap)
    args = (status if with_status else None, model if with_model else None,
            scale if with_scale else None)  # fmt: skip
    before = [None if a is None else a.copy() for a in (gains,) + args]
    got = host.InterpolateGainsHost(max_gap, smooth, normalise, 0x0F, corrections)(gains, *args)
    want = scalar_loop(gains, *args, max_gap, smooth, normalise, 0x0F, corrections)
    check(want, got, f"at {channels}, {variant}")
    for b, a in zip(before, (gains,) + args):  # no argument is modified
        assert b is None or (b.view(np.uint8) == a.view(np.uint8)).all()
    assert (got[0] is not gains) and not np.shares_memory(got[0], gains)


def test_generators_cover_the_cases():
    """Across the kinds, every outcome occurs: both status bits, filled and unfilled channels,
    held ends, and an amplitude that cannot be normalised by."""
    gains, status, model, scale, kinds = gen.make_case(5, 300, 2 * len(gen.KINDS), 4)
    assert set(kinds) == set(gen.KINDS)
    out, kept, filled, bits, amplitude = host.InterpolateGainsHost(4, 3, True)(gains, None, model)
    by_kind = dict(zip(kinds, range(len(kinds))))
    assert set(bits.tolist()) == {0, NO_DATA, GAP_LEFT}
    assert kept[by_kind["all_kept"]] == 300 and filled[by_kind["all_kept"]] == 0
    assert kept[by_kind["none_kept"]] == 0 and np.isnan(amplitude[by_kind["none_kept"]])
    assert kept[by_kind["one_kept"]] == 1 and bits[by_kind["one_kept"]] == GAP_LEFT
    assert bits[by_kind["zeros"]] == NO_DATA and amplitude[by_kind["zeros"]] == 0
    assert bits[by_kind["gap_exact"]] == 0 and filled[by_kind["gap_exact"]] == 4 * len(gen.seams(300))
    assert bits[by_kind["gap_over"]] == GAP_LEFT and filled[by_kind["gap_over"]] == 0
    assert bits[by_kind["alternating"]] == 0 and filled[by_kind["alternating"]] == 150
    # the gaps lie across the seams of the kernel
    assert gen.seams(300) == [64] and gen.seams(5000) == [64, 1024, 4096]
    assert [gen.threads_of(c) for c in (1, 64, 65, 128, 129, 1024, 1025, 16384)] == [
        64, 64, 128, 128, 256, 1024, 1024, 1024]  # fmt: skip
    for channels, gap in ((5000, 7), (5000, 8), (300, 1)):
        column, _ = gen.make_column(np.random.RandomState(1), "gap_exact", channels, gap)
        missing = np.isnan(column.real)
        for seam in gen.seams(channels):
            assert missing[seam - 1] or missing[seam]
            assert gap < 2 or (missing[seam - 1] and missing[seam])
        assert missing.sum() == gap * len(gen.seams(channels))


# --------------------------------------------------------------------------- known answers
def test_identity_on_kept_channels():
    """With smooth=1 and nothing else, out is gains bit for bit on every kept channel, zeros
    with a sign and huge values included."""
    gains, status, _, _, _ = gen.make_case(9, 200, 2 * len(gen.KINDS), 3)
    for with_status in (False, True):
        fn = host.InterpolateGainsHost(3, status_mask=0x0F)
        out, kept, filled, bits, amplitude = fn(gains, status if with_status else None)
        keep = np.isfinite(gains.real) & np.isfinite(gains.imag)
        if with_status:
            keep &= ((status & 0x0F) == 0)[:, np.newaxis]
        assert amplitude is None and (kept == keep.sum(axis=0)).all()
        assert (out.view(np.uint64)[keep] == gains.view(np.uint64)[keep]).all()
        assert keep.any(axis=0).sum() > len(gen.KINDS)


def test_constant_column_comes_back_constant():
    value = np.complex64(0.75 - 1.5j)
    gains = np.full((40, 2), value)
    for hole in (slice(0, 3), slice(5, 6), slice(10, 14), slice(20, 28), slice(37, 40)):
        gains[hole, 0] = NAN
    gains[::2, 1] = NAN
    for smooth in (1, 3, 7):
        out, kept, filled, bits, _ = host.InterpolateGainsHost(8, smooth)(gains)
        assert (out == value).all() and bits.tolist() == [0, 0]
        assert kept.tolist() == [21, 20] and filled.tolist() == [19, 20]
    # normalised: unit amplitude, the same phase, and again one value everywhere
    out, _, _, _, amplitude = host.InterpolateGainsHost(8, normalise=True)(gains)
    assert np.abs(amplitude / np.abs(value) - 1).max() < 4e-7
    assert np.abs(out - value / np.abs(value)).max() < 4e-7
    assert (out[:, 0] == out[0, 0]).all() and (out[:, 1] == out[1, 1]).all()


def test_linear_column_is_reproduced_exactly():
    """Integers linear in c, gaps between kept channels a power of two apart: t, the product
    and the sum are all exact."""
    c = np.arange(64)
    truth = (3 * c - 40 + 1j * (100 - 2 * c)).astype(np.complex64)
    gains = truth[:, np.newaxis].copy()
    for start, stop in ((1, 2), (5, 8), (10, 17), (20, 35), (40, 41), (50, 53)):
        gains[start:stop] = NAN
        assert (stop - start + 1) & (stop - start) == 0
    out, kept, filled, bits, _ = host.InterpolateGainsHost(15)(gains)
    assert_same(truth[:, np.newaxis], out)
    assert (kept[0], filled[0], bits[0]) == (64 - 30, 30, 0)
    # the ends hold the nearest value
    gains[:4] = NAN
    gains[60:] = NAN
    out = host.InterpolateGainsHost(15)(gains)[0]
    assert (out[:4] == truth[4]).all() and (out[60:] == truth[59]).all()
    assert_same(truth[4:60, np.newaxis], out[4:60])


@pytest.mark.parametrize("max_gap", [0, 1, 2, 7])
def test_gap_of_max_gap_and_one_more(max_gap):
    """A gap of exactly max_gap is filled and one of max_gap + 1 is left with bit 1: in the
    interior, at the start and at the end of the band."""
    channels = 64
    base = (1 + np.arange(channels) / 64).astype(np.complex64)

    def run(start, length):
        gains = base[:, np.newaxis].copy()
        gains[start : start + length] = NAN
        out, kept, filled, bits, _ = host.InterpolateGainsHost(max_gap)(gains)
        assert kept[0] == channels - length
        return np.isnan(out[:, 0].real), int(filled[0]), int(bits[0])

    for start in (20, 0, channels - max_gap):  # the interior, the start, the end
        left, filled, bits = run(start, max_gap)
        assert not left.any() and (filled, bits) == (max_gap, 0), start
    for start in (20, 0, channels - max_gap - 1):
        left, filled, bits = run(start, max_gap + 1)
        assert bits == GAP_LEFT, start
        if start == 20:  # an interior gap is filled whole or not at all
            assert filled == 0 and left[start : start + max_gap + 1].all() and left.sum() == max_gap + 1
        else:  # an end holds the nearest value for max_gap channels and no further
            assert filled == max_gap and left.sum() == 1
            assert left[0 if start == 0 else channels - 1]


def test_fill_status_bits():
    gains = np.ones((8, 4), np.complex64)
    gains[:, 0] = NAN  # nothing kept
    gains[2:6, 1] = NAN  # a gap that is too long
    gains[:, 3] = 0  # nothing to normalise by
    out, kept, filled, bits, amplitude = host.InterpolateGainsHost(3, normalise=True)(gains)
    assert bits.tolist() == [NO_DATA, GAP_LEFT, 0, NO_DATA]
    assert kept.tolist() == [0, 4, 8, 8] and filled.tolist() == [0, 0, 0, 0]
    assert np.isnan(out[:, 0]).all() and np.isnan(out[:, 3]).all() and np.isnan(out[2:6, 1]).all()
    assert np.isnan(amplitude[0]) and amplitude[1:].tolist() == [1, 1, 0]
    assert (host.InterpolateGainsHost.NO_DATA, host.InterpolateGainsHost.GAP_LEFT) == (1, 2)
    # status takes a channel away from every input; a masked-out bit does not
    status = np.array([0, 1, 2, 0, 0, 0, 0, 0], np.uint8)
    out, kept, filled, bits, _ = host.InterpolateGainsHost(1, status_mask=1)(gains, status)
    assert kept.tolist() == [0, 3, 7, 7] and filled.tolist() == [0, 0, 1, 1]


def test_scale_and_corrections():
    gains = np.array([[2 + 0j], [NAN], [0 + 4j]], np.complex64)
    scale = np.array([0.5j], np.complex64)
    out = host.InterpolateGainsHost(1)(gains, scale=scale)[0]
    assert out[:, 0].tolist() == [1j, -1 + 0.5j, -2]
    out = host.InterpolateGainsHost(1, corrections=True)(gains, scale=scale)[0]
    assert (out[:, 0] == np.array([-1j, -0.8 - 0.4j, -0.5], np.complex64)).all()
    # a zero or NaN scale: nothing to invert, but the column was filled
    for bad in (0, NAN):
        out, _, filled, bits, _ = host.InterpolateGainsHost(1, corrections=True)(
            gains, scale=np.array([bad], np.complex64))
        assert np.isnan(out).all() and filled[0] == 1 and bits[0] == 0


# --------------------------------------------------------------------------------- accuracy
PERIOD = 1024


def smooth_case(max_hole, delay=0.0):
    """(samples of f(c) exp(2 pi i delay c) as complex64 with holes of 1 .. max_hole channels,
    the model of the delay as complex64, the truth as complex128)."""
    rs = np.random.RandomState(max_hole)
    c = np.arange(PERIOD)
    rotation = np.exp(2j * np.pi * ((delay * c) % 1.0))
    truth = gen.bandpass(PERIOD, PERIOD) * rotation
    gains = truth.astype(np.complex64)[:, np.newaxis].copy()
    at = 3
    while at + max_hole < PERIOD - 1:
        length = rs.randint(1, max_hole + 1) if at > 3 else max_hole
        gains[at : at + length] = NAN
        at += length + rs.randint(1, 5)
    return gains, rotation.astype(np.complex64)[:, np.newaxis], truth


def accuracy_bound(max_hole):
    """Linear interpolation between samples h = max_hole + 1 apart is off by at most
    h^2 / 8 max|f''|; the float32 steps (the rounding of the samples and of the model, two
    rotations and the interpolation itself) are given 8 units of 2^-23 max|f|."""
    curvature = gen.bandpass_curvature(PERIOD)
    return (max_hole + 1) ** 2 / 8 * curvature + 8 * 2.0**-23 * np.abs(gen.bandpass(PERIOD, PERIOD)).max()


@pytest.mark.parametrize("max_hole", [1, 4, 16, 64])
def test_accuracy_on_a_smooth_bandpass(max_hole):
    gains, _, truth = smooth_case(max_hole)
    out, kept, filled, bits, _ = host.InterpolateGainsHost(max_hole)(gains)
    assert bits[0] == 0 and filled[0] > PERIOD // 4 and kept[0] + filled[0] == PERIOD
    error = np.abs(out[:, 0].astype(np.complex128) - truth).max()
    print(f"holes of up to {max_hole}: error {error:.3e}, bound {accuracy_bound(max_hole):.3e}")
    assert error <= accuracy_bound(max_hole)


@pytest.mark.parametrize("max_hole", [1, 4, 16, 64])
def test_the_model_is_what_makes_a_delay_harmless(max_hole):
    """The same bandpass under a delay of 0.2 turns per channel: with the delay's model it
    meets the same bound, without it linear interpolation of the wound phase misses the bound
    by more than a factor of 100."""
    gains, model, truth = smooth_case(max_hole, 0.2)
    fn = host.InterpolateGainsHost(max_hole)
    out, _, filled, bits, _ = fn(gains, model=model)
    assert bits[0] == 0 and filled[0] > PERIOD // 4
    error = np.abs(out[:, 0].astype(np.complex128) - truth).max()
    plain = np.abs(fn(gains)[0][:, 0].astype(np.complex128) - truth).max()
    bound = accuracy_bound(max_hole)
    print(f"holes of up to {max_hole}: error {error:.3e} with the model, {plain:.3e} without, "
          f"bound {bound:.3e}")  # fmt: skip
    assert error <= bound
    assert plain > 100 * bound


# ----------------------------------------------------------------------------------- errors
def test_host_errors():
    for bad in (-1, 16385):
        with pytest.raises(ValueError, match="max_gap"):
            host.InterpolateGainsHost(bad)
    for bad in (1.0, True, "3", None):
        with pytest.raises(TypeError, match="max_gap"):
            host.InterpolateGainsHost(bad)
    for bad in (0, 2, 4, 30, 33, -1):
        with pytest.raises(ValueError, match="smooth"):
            host.InterpolateGainsHost(1, bad)
    for bad in (3.0, False):
        with pytest.raises(TypeError, match="smooth"):
            host.InterpolateGainsHost(1, bad)
    for bad in (-1, 256):
        with pytest.raises(ValueError, match="status_mask"):
            host.InterpolateGainsHost(1, status_mask=bad)
    with pytest.raises(TypeError, match="status_mask"):
        host.InterpolateGainsHost(1, status_mask=1.0)
    fn = host.InterpolateGainsHost(np.int64(16384), np.int32(31))
    assert (fn.max_gap, fn.smooth, fn.normalise, fn.status_mask, fn.corrections) == (
        16384, 31, False, 255, False)  # fmt: skip
    fn = host.InterpolateGainsHost(0, 1, 1, 0, 1)
    assert (fn.max_gap, fn.normalise, fn.status_mask, fn.corrections) == (0, True, 0, True)
    assert (host.InterpolateGainsHost.MAX_CHANNELS, host.InterpolateGainsHost.MAX_GAP,
            host.InterpolateGainsHost.MAX_SMOOTH) == (16384, 16384, 31)  # fmt: skip
    good, status, model, scale, _ = gen.make_case(1, 6, 3, 2)
    fn(good, status, model, scale)
    for bad in (good.astype(np.complex128), good[0], good[:0], good[:, :0], good.real,
                np.zeros((16385, 1), np.complex64)):  # fmt: skip
        with pytest.raises(ValueError, match="gains"):
            fn(bad, status, model, scale)
    for bad in (status.astype(np.int8), status[:5], status[:, np.newaxis], np.zeros(7, np.uint8)):
        with pytest.raises(ValueError, match="status"):
            fn(good, bad)
    for bad in (model.astype(np.complex128), model[:5], model[:, :2], model[:, 0], model.real):
        with pytest.raises(ValueError, match="model"):
            fn(good, model=bad)
    for bad in (scale.astype(np.complex128), scale[:2], scale[:, np.newaxis], scale.real):
        with pytest.raises(ValueError, match="scale"):
            fn(good, scale=bad)
    fn(np.zeros((16384, 1), np.complex64))
    for bad in ((0, 1), (16385, 1), (4, 0)):
        with pytest.raises(ValueError):
            fn.check_shape(*bad)


def test_template_and_operation_errors(context, queue):
    with pytest.raises(ValueError):
        ingest.InterpolateGainsTemplate(context, 8, tuning={"wgs": 256})
    assert ingest.InterpolateGainsTemplate(context, 8, tuning={}).tuning == {}
    assert ingest.InterpolateGainsTemplate.autotune(context) == {}
    assert ingest.InterpolateGainsTemplate.TUNING_KEYS == ()
    assert ingest.InterpolateGainsTemplate.host_class is host.InterpolateGainsHost
    assert ingest.InterpolateGainsTemplate.KERNEL == "ksp_interpolate_gains"
    assert ingest.InterpolateGainsTemplate.operation_class is ingest.InterpolateGains
    for name, bads in (("max_gap", (-1, 16385)), ("smooth", (0, 2, 33)), ("status_mask", (-1, 256))):
        for bad in bads:
            with pytest.raises(ValueError, match=name):
                ingest.InterpolateGainsTemplate(context, **{"max_gap": 8, name: bad})
    for name in ("max_gap", "smooth", "status_mask"):
        with pytest.raises(TypeError, match=name):
            ingest.InterpolateGainsTemplate(context, **{"max_gap": 8, name: 1.5})
    template = ingest.InterpolateGainsTemplate(context, 8)
    assert template.kernel.name == "ksp_interpolate_gains"
    assert (template.max_gap, template.smooth, template.normalise, template.status,
            template.status_mask, template.model, template.scale, template.corrections) == (
        8, 1, False, True, 255, True, False, False)  # fmt: skip
    for args in [(0, 4), (-1, 4), (16385, 4), (4, 0), (4, -1)]:
        with pytest.raises(ValueError):
            template.instantiate(queue, *args)
    assert isinstance(template.instantiate(queue, 16384, 1), ingest.InterpolateGains)
    fn = ingest.InterpolateGainsTemplate(context, 5, 9, True, False, 0x30, False, True,
                                         True).instantiate(queue, 100, 7)  # fmt: skip
    assert fn.parameters() == {"max_gap": 5, "smooth": 9, "normalise": True, "status": False,
                               "status_mask": 0x30, "model": False, "scale": True,
                               "corrections": True, "channels": 100, "n_inputs": 7}  # fmt: skip


def test_host_from_device(context, queue):
    gains, status, model, scale, _ = gen.make_case(1, 10, 5, 2)
    for with_status, with_model, with_scale, normalise, corrections in VARIANTS:
        template = ingest.InterpolateGainsTemplate(context, 2, 3, normalise, with_status, 0xFF,
                                                   with_model, with_scale, corrections)  # fmt: skip
        adapter = ingest.InterpolateGainsHostFromDevice(template, queue)
        del queue.launches[:]
        given = dict(status=status if with_status else None, model=model if with_model else None,
                     scale=scale if with_scale else None)  # fmt: skip
        out = adapter(gains, **given)
        assert len(out) == 5 and (out[4] is not None) == normalise
        for o, shape, dtype in zip(out, [(10, 5)] + [(5,)] * 4,
                                   (np.complex64, np.int32, np.int32, np.uint8, f32)):  # fmt: skip
            assert o is None or (o.shape, o.dtype) == (shape, dtype)
        assert [name for name, _ in queue.launches] == ["ksp_interpolate_gains"]
        assert [int(a) for a in queue.launches[0][1][9:11]] == [10, 5]
        for name, present in (("status", with_status), ("model", with_model), ("scale", with_scale)):
            wrong = dict(given)
            wrong[name] = None if present else {"status": status, "model": model, "scale": scale}[name]
            with pytest.raises(TypeError, match=name):
                adapter(gains, **wrong)
    adapter = ingest.InterpolateGainsHostFromDevice(
        ingest.InterpolateGainsTemplate(context, 2, status=False, model=False), queue)
    with pytest.raises(ValueError):
        adapter(gains[:0])


# ----------------------------------------------------------------------------------- wiring
@pytest.mark.parametrize("with_status, with_model, with_scale, normalise, corrections", VARIANTS)
def test_slots_and_launch_arguments(with_status, with_model, with_scale, normalise, corrections,
                                    context, queue):  # fmt: skip
    template = ingest.InterpolateGainsTemplate(context, 11, 5, normalise, with_status, 0x3C,
                                               with_model, with_scale, corrections)  # fmt: skip
    fn = template.instantiate(queue, 300, 58)
    names = (["gains"] + (["status"] if with_status else []) + (["model"] if with_model else [])
             + (["scale"] if with_scale else []) + ["out", "kept", "filled", "fill_status"]
             + (["mean_amplitude"] if normalise else []))  # fmt: skip
    assert list(fn.slots) == names
    shapes = {"gains": ((300, 58), np.complex64), "status": ((300,), np.uint8),
              "model": ((300, 58), np.complex64), "scale": ((58,), np.complex64),
              "out": ((300, 58), np.complex64), "kept": ((58,), np.int32),
              "filled": ((58,), np.int32), "fill_status": ((58,), np.uint8),
              "mean_amplitude": ((58,), f32)}  # fmt: skip
    for name, slot in fn.slots.items():
        assert (slot.shape, slot.dtype) == shapes[name], name
    # a dimension object of its own for everything that can be padded
    dims = [d for slot in fn.slots.values() for d in slot.dimensions]
    assert len({id(d) for d in dims}) == len(dims) == len(fn.slots) + 2 + with_model
    accel.Dimension(58, min_padded_size=100).link(fn.slots["gains"].dimensions[1])
    accel.Dimension(58, min_padded_size=150).link(fn.slots["out"].dimensions[1])
    if with_model:
        accel.Dimension(58, min_padded_size=200).link(fn.slots["model"].dimensions[1])
    fn()
    assert [name for name, _ in queue.launches] == ["ksp_interpolate_gains"]
    args = queue.launches[0][1]
    assert len(args) == 18
    order = ["gains", "status", "model", "scale", "out", "kept", "filled", "fill_status",
             "mean_amplitude"]  # fmt: skip
    for got, name in zip(args[:9], order):
        assert got is (fn.buffer(name).buffer if name in names else None), name
    assert all(isinstance(a, np.int32) for a in args[9:])
    assert [int(a) for a in args[9:11]] == [300, 58]
    assert int(args[11]) == fn.buffer("gains").padded_shape[1] == 112  # whole 128-byte rows
    assert int(args[12]) == (fn.buffer("model").padded_shape[1] if with_model else 0)
    assert int(args[12]) == (208 if with_model else 0)
    assert int(args[13]) == fn.buffer("out").padded_shape[1] == 160
    assert [int(a) for a in args[14:]] == [11, 5, 0x3C, int(corrections)]


def test_in_place_binding(context, queue):
    """out bound to the buffer of gains: the launcher gets the same pointer and stride twice."""
    fn = ingest.InterpolateGainsTemplate(context, 4, status=False, model=False).instantiate(
        queue, 20, 6)  # fmt: skip
    fn.ensure_all_bound()
    fn.bind(out=fn.buffer("gains"))
    fn()
    args = queue.launches[0][1]
    assert args[0] is args[4] is fn.buffer("gains").buffer and int(args[11]) == int(args[13])


def test_between_fit_and_apply(context, queue):
    """solve_gains -> fit_delays -> interpolate_gains -> apply_gains: the new step reads the
    solver's gains and status and fit's model, and apply_gains multiplies by its out."""
    rows, baselines, n_inputs = 64, 66, 12
    solve = ingest.SolveGainsTemplate(context).instantiate(queue, rows, baselines, n_inputs)
    fit = ingest.FitDelaysTemplate(context, 1e6).instantiate(queue, rows, n_inputs)
    interp = ingest.InterpolateGainsTemplate(context, 8, corrections=True).instantiate(
        queue, rows, n_inputs)  # fmt: skip
    apply_gains = ingest.ApplyGainsTemplate(context).instantiate(queue, rows, baselines, n_inputs)
    accel.Dimension(n_inputs, min_padded_size=40).link(solve.slots["gains"].dimensions[1])
    accel.Dimension(n_inputs, min_padded_size=70).link(apply_gains.slots["gains"].dimensions[1])
    accel.Dimension(n_inputs, min_padded_size=90).link(fit.slots["model"].dimensions[1])
    seq = accel.OperationSequence(
        queue, [("solve", solve), ("fit", fit), ("interp", interp), ("apply_gains", apply_gains)],
        compounds={"vis": ["solve:vis", "apply_gains:vis"],
                   "weights": ["solve:weights", "apply_gains:weights"],
                   "flags": ["solve:flags", "apply_gains:flags"],
                   "gains": ["solve:gains", "fit:gains", "interp:gains"],
                   "status": ["solve:status", "fit:status", "interp:status"],
                   "k": ["fit:model", "interp:model"],
                   "corr": ["interp:out", "apply_gains:gains"]})  # fmt: skip
    assert {"gains", "status", "k", "corr", "interp:kept", "interp:filled",
            "interp:fill_status"} <= set(seq.slots)  # fmt: skip
    seq()
    assert [name for name, _ in queue.launches] == [
        "ksp_solve_gains", "ksp_fit_delays", "ksp_interpolate_gains", "ksp_apply_gains"]  # fmt: skip
    solve_args, fit_args, interp_args, apply_args = (launch[1] for launch in queue.launches)
    assert solve_args[5] is fit_args[0] is interp_args[0] is seq.buffer("gains").buffer
    assert solve_args[7] is fit_args[1] is interp_args[1] is seq.buffer("status").buffer
    assert fit_args[6] is interp_args[2] is seq.buffer("k").buffer
    assert interp_args[4] is apply_args[3] is seq.buffer("corr").buffer
    assert int(interp_args[11]) == seq.buffer("gains").padded_shape[1] == 48
    assert int(interp_args[12]) == int(fit_args[10]) == seq.buffer("k").padded_shape[1] == 96
    assert int(interp_args[13]) == int(apply_args[14]) == 80
    assert [int(a) for a in interp_args[9:11]] == [rows, n_inputs]
    assert [int(a) for a in interp_args[14:]] == [8, 1, 255, 1]


# ------------------------------------------------------------------- the launcher's checks
@pytest.fixture(scope="module")
def lib():
    from katsdpsigproc_amd import _lib, build_native

    if not os.path.exists(_lib.LIB_PATH):
        build_native.build()
    return _lib.load()


POINTERS = ["gains", "status", "model", "scale", "out", "kept", "filled", "fill_status",
            "mean_amplitude"]  # fmt: skip
NUMBERS = ["channels", "n_inputs", "gains_stride", "model_stride", "out_stride", "max_gap",
           "smooth", "status_mask", "corrections"]  # fmt: skip


def test_argument_validation_without_gpu(lib):
    from katsdpsigproc_amd import _lib

    # never dereferenced: every call below fails its checks first. Nine arrays far apart.
    p = {name: ctypes.c_void_p((i + 1) << 32) for i, name in enumerate(POINTERS)}
    good = dict(channels=4, n_inputs=8, gains_stride=8, model_stride=8, out_stride=8, max_gap=2,
                smooth=3, status_mask=255, corrections=0)  # fmt: skip

    def call(device=0, **changed):
        a = dict(p, **good)
        a.update(changed)
        rc = lib.ksp_interpolate_gains(device, None, *(a[name] for name in POINTERS),
                                       *(a[name] for name in NUMBERS))  # fmt: skip
        assert rc != 0
        return _lib.last_error()

    for name in ("gains", "out", "kept", "filled", "fill_status"):
        assert f"invalid argument: {name} is NULL" in call(**{name: None})
    for bad in (0, -1, 16385):
        assert "invalid argument: channels must be 1..16384" in call(channels=bad)
    for bad in (0, -1):
        assert "invalid argument: n_inputs must be at least 1" in call(n_inputs=bad)
    for bad in (-1, 16385):
        assert "invalid argument: max_gap must be 0..16384" in call(max_gap=bad)
    for bad in (0, -1, 2, 30, 32, 33):
        assert "invalid argument: smooth must be odd and 1..31" in call(smooth=bad)
    for bad in (-1, 256):
        assert "invalid argument: status_mask must be 0..255" in call(status_mask=bad)
    for bad in (-1, 2):
        assert "invalid argument: corrections must be 0 or 1" in call(corrections=bad)
    for name in ("gains", "model", "out"):
        assert f"invalid argument: {name}_stride is smaller than n_inputs" in call(
            **{name + "_stride": 7})
    # the order of the checks: everything wrong at once, then one thing fewer at a time
    wrong = dict(channels=0, n_inputs=0, gains_stride=-1, model_stride=-1, out_stride=-1,
                 max_gap=-1, smooth=2, status_mask=-1, corrections=2)  # fmt: skip
    nulls = dict.fromkeys(p)
    for name in ("gains", "out", "kept", "filled", "fill_status"):
        assert f"invalid argument: {name} is NULL" in call(**nulls, **wrong)
        nulls[name] = p[name]
    order = [("channels", "channels must be"), ("n_inputs", "n_inputs must be"),
             ("max_gap", "max_gap must be"), ("smooth", "smooth must be"),
             ("status_mask", "status_mask must be"), ("corrections", "corrections must be"),
             ("gains_stride", "gains_stride is smaller"), ("model_stride", "model_stride is smaller"),
             ("out_stride", "out_stride is smaller")]  # fmt: skip
    overlapping = dict(out=ctypes.c_void_p(p["gains"].value + 8), model=p["gains"])
    for name, message in order:
        assert message in call(**wrong, **overlapping), name
        wrong[name] = good[name]
    assert "out overlaps gains" in call(**overlapping)
    # an absent array's stride is not looked at, and every optional array may be absent
    assert "hipSetDevice(device) failed" in call(device=-1, model=None, model_stride=-1)
    assert "hipSetDevice(device) failed" in call(device=-1, status=None, scale=None,
                                                 mean_amplitude=None)  # fmt: skip

    def at(name, offset):
        return ctypes.c_void_p(p[name].value + offset)

    extent = (3 * 8 + 8) * 8  # the bytes from the first element to the last
    message = "invalid argument: out overlaps gains without being gains with the same stride"
    assert message in call(out=at("gains", extent - 1))
    assert message in call(out=at("gains", -(extent - 1)))
    assert message in call(out=p["gains"], out_stride=9)
    assert message in call(out=at("gains", 8))
    assert "invalid argument: out overlaps model" in call(out=p["model"])
    assert "invalid argument: out overlaps model" in call(out=at("model", extent - 1))
    assert "invalid argument: out overlaps model" in call(out=at("model", -(extent - 1)))
    assert "invalid argument: out overlaps model" in call(out=p["gains"], model=p["gains"])
    # in place, arrays that only touch and the limits pass every check: what is left to fail is
    # the first device call, which device -1 fails on any machine
    for passing in (dict(out=p["gains"]), dict(out=at("gains", extent)), dict(out=at("gains", -extent)),
                    dict(out=at("model", extent)), dict(out=at("model", -extent)),
                    dict(out=p["model"], model=None), dict(channels=16384, max_gap=16384, smooth=31),
                    dict(channels=1, max_gap=0, smooth=1, status_mask=0, corrections=1)):  # fmt: skip
        assert "hipSetDevice(device) failed" in call(device=-1, **passing)


def test_header_binding_and_exports(lib):
    from katsdpsigproc_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "katsdpsigproc_hip.h")).read()
    comment = re.search(r"/\* interpolate_gains:.*?\*/", text, re.S).group(0)
    assert "InterpolateGainsHost" in comment
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declaration = re.search(r"int ksp_interpolate_gains\((.*?)\);", text, re.S)
    assert declaration is not None
    parameters = [" ".join(part.split()) for part in declaration.group(1).split(",")]
    argtypes = _lib.SIGNATURES["ksp_interpolate_gains"]
    assert len(parameters) == len(argtypes) == 20
    for parameter, argtype in zip(parameters, argtypes):
        assert ("*" in parameter) == (argtype is ctypes.c_void_p), parameter
        assert argtype in (ctypes.c_int, ctypes.c_void_p)
    names = [parameter.replace("*", " ").split()[-1] for parameter in parameters]
    assert names == ["device", "stream"] + POINTERS + NUMBERS
    assert hasattr(lib, "ksp_interpolate_gains")
    assert "ksp_interpolate_gains" in _lib.declared_symbols()
    assert lib.ksp_abi_version() == _lib.ABI_VERSION == 5
    for name in ("InterpolateGainsTemplate", "InterpolateGains", "InterpolateGainsHostFromDevice"):
        assert hasattr(ingest, name)
    assert hasattr(host, "InterpolateGainsHost")
