"""Fitting per-input delays without a GPU: ``rfi.host.FitDelaysHost`` against a loop of float32
and float64 scalars, its transform against ``np.fft``, known answers, the accuracy against the
generating tones and against a float64 restatement of the estimator, solve -> fit -> apply on
model data; argument errors, slot lists and every launch argument of every variant on the fake
backend, the sequence solve_gains -> fit_delays -> apply_gains, and the argument checks of
``ksp_fit_delays``, which come before any device call."""

import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from katsdpsigproc_amd import accel
from katsdpsigproc_amd.rfi import host, ingest
from tests import inputs_fit_delays as gen
from tests.fakes import FakeContext
from tests.inputs_fit_delays import assert_same
from tests.test_predict import scalar_cos_sin

f32, f64 = np.float32, np.float64
#: (status, model, corrections) of every variant of the operation
VARIANTS = list(itertools.product([True, False], repeat=3))
OUTPUTS = ("delays", "phasors", "amplitudes", "fit_status", "model")
NO_FIT, STEP_REJECTED = 1, 2


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


def scalar_transform(x, n_fft):
    """The transform of the class docstring on a list of (float32, float32)."""
    bits = n_fft.bit_length() - 1
    a = [x[int(format(i, f"0{bits}b")[::-1], 2)] for i in range(n_fft)]
    for s in range(1, bits + 1):
        half = 1 << (s - 1)
        for start in range(0, n_fft, 2 * half):
            for j in range(half):
                co, si = scalar_cos_sin(j / (1 << s))
                tw_re, tw_im = f32(co), f32(-si)
                (a_re, a_im), (b_re, b_im) = a[start + j], a[start + j + half]
                bt_re = b_re * tw_re - b_im * tw_im
                bt_im = b_re * tw_im + b_im * tw_re
                a[start + j] = (a_re + bt_re, a_im + bt_im)
                a[start + j + half] = (a_re - bt_re, a_im - bt_im)
    return a


def scalar_sums(x, kept, c_pad, nu):
    terms = [[f64(0)] * c_pad for _ in range(6)]
    for c in range(len(x)):
        if not kept[c]:
            continue
        co, si = scalar_cos_sin(float(c) * float(nu))
        x_re, x_im = f64(x[c][0]), f64(x[c][1])
        e_re = x_re * f64(co) + x_im * f64(si)
        e_im = x_im * f64(co) - x_re * f64(si)
        cc = f64(c)
        for i, value in enumerate((e_re, e_im, cc * e_re, cc * e_im, (cc * cc) * e_re,
                                   (cc * cc) * e_im)):  # fmt: skip
            terms[i][c] = value
    return [scalar_tree(t) for t in terms]


def scalar_loop(gains, status, width, n_fft, refine, mask, corrections):
    """FitDelaysHost as a loop over inputs, channels and butterflies of np.float32 and
    np.float64 scalars, one operation at a time."""
    channels, n_inputs = gains.shape
    nan32 = f32(np.nan)
    delays = np.empty(n_inputs, f64)
    phasors = np.empty(n_inputs, np.complex64)
    amplitudes = np.empty(n_inputs, f32)
    fit_status = np.zeros(n_inputs, np.uint8)
    model = np.empty((channels, n_inputs), np.complex64)
    c_pad = 1
    while c_pad < channels:
        c_pad *= 2
    for p in range(n_inputs):
        x = [(f32(0), f32(0))] * n_fft
        kept = [False] * channels
        for c in range(channels):
            re, im = f32(gains[c, p].real), f32(gains[c, p].imag)
            kept[c] = bool(np.isfinite(re) and np.isfinite(im)
                           and (status is None or int(status[c]) & mask == 0))  # fmt: skip
            if kept[c]:
                x[c] = (re, im)
        n_kept = sum(kept)
        peak, k0 = None, None
        for k, (re, im) in enumerate(scalar_transform(x, n_fft)):
            power = re * re + im * im
            assert isinstance(power, f32)
            if not np.isnan(power) and (peak is None or power > peak):
                peak, k0 = power, k
        no_fit = n_kept < 2 or peak is None or not (0 < peak < np.inf)
        bits = 0
        if not no_fit:
            nu = f64(k0) / f64(n_fft)
            for _ in range(refine):
                d0r, d0i, d1r, d1i, d2r, d2i = scalar_sums(x[:channels], kept, c_pad, nu)
                num = d1i * d0r - d1r * d0i
                den = f64(6.283185307179586) * ((d1r * d1r + d1i * d1i) - (d2r * d0r + d2i * d0i))
                step = num / den
                assert isinstance(step, f64)
                if den < 0 and abs(step) <= 1.0 / n_fft:
                    nu = nu - step
                else:
                    bits |= STEP_REJECTED
                    break
            d0r, d0i = scalar_sums(x[:channels], kept, c_pad, nu)[:2]
            m = np.sqrt(d0r * d0r + d0i * d0i)
            no_fit = not (0 < m < np.inf)
        if no_fit:
            delays[p], phasors[p], amplitudes[p] = np.nan, complex(np.nan, np.nan), nan32
            model[:, p] = complex(np.nan, np.nan)
            fit_status[p] = bits | NO_FIT
            continue
        ph_re, ph_im = f32(d0r / m), f32(d0i / m)
        phasors[p] = complex(ph_re, ph_im)
        amplitudes[p] = f32(m / f64(n_kept))
        delays[p] = (nu - np.rint(nu)) / f64(width)
        fit_status[p] = bits
        for c in range(channels):
            co, si = scalar_cos_sin(float(c) * float(nu))
            re = f32(f64(ph_re) * f64(co) - f64(ph_im) * f64(si))
            im = f32(f64(ph_re) * f64(si) + f64(ph_im) * f64(co))
            model[c, p] = complex(re, -im if corrections else im)
    return delays, phasors, amplitudes, fit_status, model


@pytest.mark.parametrize("channels, n_fft, refine, with_status, corrections", [
    (1, 4, 3, False, False), (2, 4, 3, True, False), (2, 8, 1, False, True),
    (3, 8, 3, True, True), (5, 16, 8, False, False), (16, 32, 2, True, False),
    (13, 64, 3, True, True), (24, 64, 0, False, False)])  # fmt: skip
def test_host_against_scalar_loop(channels, n_fft, refine, with_status, corrections):
    n_inputs = 2 * len(gen.KINDS)
    gains, _, _ = gen.make_gains(channels + n_fft, channels, n_inputs, n_fft)
    status = gen.make_status(channels, channels, 0x0F) if with_status else None
    fn = host.FitDelaysHost(-2.5e5, n_fft, refine, 0x0F, corrections)
    before = gains.copy()
    got = fn(gains, status)
    with np.errstate(all="ignore"):
        want = scalar_loop(gains, status, -2.5e5, n_fft, refine, 0x0F, corrections)
    assert_same(before, gains, "gains")
    for name, w, g in zip(OUTPUTS, want, got):
        assert_same(w, g, name)
    if channels >= 5:
        assert set(got[3].tolist()) >= ({0, NO_FIT} | ({STEP_REJECTED} if refine else set()))


# ------------------------------------------------------------------------------ the transform
@pytest.mark.parametrize("channels, n_fft", [(1, 4), (2, 4), (4, 8), (25, 64), (100, 256),
                                             (1000, 4096), (8192, 16384)])  # fmt: skip
def test_transform_against_numpy(channels, n_fft):
    """Against np.fft.fft of the same padded columns in float64. An element passes through
    log2(n_fft) butterflies, and each adds at most four float32 roundings of its magnitude (the
    twiddle's, which is within 2^-24 sqrt(2) of the unit circle, the two of a product and its
    sum, and the one of the add), so |X[k] - exact| <= 4 log2(n_fft) 2^-24 sum |x[c]|."""
    n_inputs = 8
    gains, _, _ = gen.make_gains(n_fft, channels, n_inputs, n_fft, kinds=gen.KINDS[:8])
    x = np.zeros((n_fft, n_inputs), np.complex64)
    x[:channels] = np.where(np.isfinite(gains.real) & np.isfinite(gains.imag), gains, 0)
    re, im = host.FitDelaysHost.transform(np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag))
    assert re.dtype == im.dtype == f32 and re.shape == im.shape == x.shape
    want = np.fft.fft(x.astype(np.complex128), axis=0)
    norm = np.abs(x.astype(np.complex128)).sum(axis=0)
    error = np.abs((re.astype(f64) + 1j * im.astype(f64)) - want).max(axis=0)
    bound = 4 * np.log2(n_fft) * 2.0**-24 * norm
    assert (error <= bound).all(), (error / norm).max()
    if channels > 1:
        assert (error > 0).any()


# ------------------------------------------------------------------------------ known answers
def quarter_tone(channels, turns=0.25, amplitude=1.0):
    """1, i, -1, -i, ... (or its conjugate for -0.25): every value exact in float32."""
    values = np.array([1, 1j, -1, -1j] if turns > 0 else [1, -1j, -1, 1j], np.complex64)
    return (amplitude * values[np.arange(channels) % 4])[:, np.newaxis].astype(np.complex64)


@pytest.mark.parametrize("channels, n_fft", [(8, 16), (8, 32), (12, 64), (100, 1024)])
def test_exact_bin_tone(channels, n_fft):
    """A tone on a bin whose samples and phasors are exact: every step is exactly 0, so any
    number of them leaves nu = k / n_fft, and the model is the tone."""
    gains = quarter_tone(channels, 0.25, 3.0)
    results = [host.FitDelaysHost(2e5, n_fft, refine)(gains) for refine in (0, 1, 8)]
    for delays, phasors, amplitudes, fit_status, model in results:
        assert fit_status.tolist() == [0]
        assert delays[0] == (n_fft // 4) / (n_fft * 2e5) == 0.25 / 2e5
        assert phasors[0] == 1 and amplitudes[0] == 3
        assert np.array_equal(model, quarter_tone(channels))  # (the sign of a zero aside)
    # a whole number of turns away it is the same tone
    assert host.FitDelaysHost(2e5, n_fft)(quarter_tone(channels, -0.25))[0][0] == -0.25 / 2e5


def test_signs():
    """A negative nu comes out negative, and a negative channel_width (a band stored in
    descending frequency) turns the sign of the delay but nothing else."""
    gains = quarter_tone(16, -0.25)
    up = host.FitDelaysHost(1e6, 64)(gains)
    down = host.FitDelaysHost(-1e6, 64)(gains)
    assert up[0][0] == -0.25e-6 and down[0][0] == 0.25e-6
    for a, b in zip(up[1:], down[1:]):
        assert_same(a, b)
    # a tone off the bins: the sign of the generating nu, either way
    for nu in (-0.1234, 0.1234, -0.4999, 0.4999):
        tone = gen.tone(50, nu).astype(np.complex64)[:, np.newaxis]
        delays = host.FitDelaysHost(-1e3)(tone)[0]
        assert abs(delays[0] * -1e3 - nu) < 1e-6


def test_too_few_channels():
    gains = quarter_tone(8)
    fn = host.FitDelaysHost(1e6)
    for kept in ([], [3], [0]):
        case = np.full((8, 1), complex(np.nan, np.nan), np.complex64)
        case[kept] = gains[kept]
        delays, phasors, amplitudes, fit_status, model = fn(case)
        assert fit_status.tolist() == [NO_FIT]
        assert np.isnan(delays).all() and np.isnan(amplitudes).all()
        assert np.isnan(phasors.real).all() and np.isnan(phasors.imag).all()
        assert np.isnan(model.real).all() and np.isnan(model.imag).all()
    # two are enough, wherever they are, and the model covers the whole band
    case = np.full((8, 1), complex(np.nan, 1.0), np.complex64)
    case[[2, 3]] = gains[[2, 3]]
    delays, phasors, amplitudes, fit_status, model = fn(case)
    assert fit_status.tolist() == [0] and amplitudes[0] == 1
    assert abs(delays[0] - 0.25e-6) < 1e-12
    assert np.abs(model - gains).max() < 1e-6
    # the same channels taken away by status
    status = np.array([1, 2, 0, 0, 4, 8, 16, 128], np.uint8)
    for a, b in zip(fn(case), fn(gains, status)):
        assert_same(a, b)
    # only the bits of the mask count
    masked = host.FitDelaysHost(1e6, status_mask=0x0F)(gains, status)
    case = gains.copy()
    case[[0, 1, 4, 5]] = np.nan
    for a, b in zip(host.FitDelaysHost(1e6)(case), masked):
        assert_same(a, b)
    none = host.FitDelaysHost(1e6, status_mask=0)(gains, np.full(8, 255, np.uint8))
    for a, b in zip(fn(gains), none):
        assert_same(a, b)


def test_fit_status_bits():
    """Bit 0: no fit. Bit 1: a step was rejected, here 0 / 0 for a single channel that is not
    zero, after which the coarse nu stands; with refine=0 no step is taken."""
    gains = np.zeros((8, 3), np.complex64)
    gains[:, 0] = quarter_tone(8)[:, 0]
    gains[0, 1] = 2 + 0j
    for refine in (0, 1, 5):
        delays, phasors, amplitudes, fit_status, model = host.FitDelaysHost(1e6, 32, refine)(gains)
        assert fit_status.tolist() == [0, STEP_REJECTED if refine else 0, NO_FIT]
        assert delays[1] == 0 and phasors[1] == 1 and amplitudes[1] == f32(2 / 8)
        assert (model[:, 1] == 1).all() and np.isnan(delays[2])
    # an overflowing transform: every power is inf or NaN
    gains = (quarter_tone(8) * f32(3e38)).astype(np.complex64)
    assert host.FitDelaysHost(1e6)(gains)[3].tolist() == [NO_FIT]


def test_refine_zero_and_more():
    """Without a step nu is the bin; steps only ever move it by up to a bin each."""
    nu = 25.37 / 256
    tone = gen.tone(64, nu).astype(np.complex64)[:, np.newaxis]
    coarse = host.FitDelaysHost(1.0, 256, 0)(tone)[0][0]
    assert coarse == 25 / 256
    errors = [abs(host.FitDelaysHost(1.0, 256, refine)(tone)[0][0] - nu) for refine in range(5)]
    assert errors[0] > 1e-3 and errors[1] < errors[0] / 10 and errors[2] < errors[1] / 10
    assert max(errors[3:]) < 1e-9


def test_corrections():
    gains, _, _ = gen.make_gains(5, 40, 36, 256)
    plain = host.FitDelaysHost(1e6, 256)(gains)
    conj = host.FitDelaysHost(1e6, 256, corrections=True)(gains)
    for a, b in zip(plain[:4], conj[:4]):
        assert_same(a, b)
    assert_same(plain[4].real.copy(), conj[4].real.copy(), "real")
    assert_same(plain[4].imag.copy(), (-conj[4].imag).copy(), "imag")
    fitted = plain[3] == 0
    assert fitted.sum() > 20 and np.abs(plain[4][:, fitted] * conj[4][:, fitted] - 1).max() < 3e-7


def test_lowest_of_equal_peaks():
    """A real, alternating column has the same power at k and n_fft - k, bit for bit: the
    lower index is the answer."""
    gains, kinds, _ = gen.make_gains(1, 40, len(gen.KINDS), 128)
    p = kinds.index("alternating")
    x = np.zeros((128, 1), np.complex64)
    x[:40, 0] = gains[:, p]
    re, im = host.FitDelaysHost.transform(np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag))
    power = (re * re + im * im)[:, 0]
    assert power[32] == power[96] == power.max() and np.argmax(power) == 32
    delays = host.FitDelaysHost(1.0, 128, 0)(gains)[0]
    assert delays[p] == 0.25


def test_generators_cover_the_cases():
    gains, kinds, nus = gen.make_gains(3, 100, 2 * len(gen.KINDS), 256)
    assert kinds[: len(gen.KINDS)] == list(gen.KINDS)
    by_kind = {kind: p for p, kind in enumerate(kinds[: len(gen.KINDS)])}
    assert nus[by_kind["zero_delay"]] == 0 and nus[by_kind["plus_half"]] == 0.5
    assert nus[by_kind["minus_half"]] == -0.5
    assert (nus[by_kind["on_bin"]] * 256) % 1 == 0 and (nus[by_kind["half_bin"]] * 256) % 1 == 0.5
    column = gains[:, by_kind["missing"]]
    assert 0 < np.isnan(column.real).sum() < 30
    assert np.isnan(gains[:, by_kind["all_nan"]].real).all()
    assert np.isfinite(gains[:, by_kind["one_kept"]].real).sum() == 1
    assert np.isfinite(gains[:, by_kind["two_kept"]].real).sum() == 2
    zeros = gains[:, by_kind["zeros"]]
    assert not zeros.any() and np.signbit(zeros.real).any() and not np.signbit(zeros.real).all()
    assert np.isinf(gains[:, by_kind["infinite"]].real).any()
    assert np.count_nonzero(gains[:, by_kind["delta"]]) == 1 and gains[0, by_kind["delta0"]] != 0
    # the huge column overflows the transform: P holds inf and NaN
    x = np.zeros((256, 1), np.complex64)
    x[:100, 0] = gains[:, by_kind["huge"]]
    with np.errstate(all="ignore"):
        re, im = host.FitDelaysHost.transform(np.ascontiguousarray(x.real), np.ascontiguousarray(x.imag))
        power = re * re + im * im
    assert np.isinf(power).any() and np.isnan(power).any()
    status = gen.make_status(1, 200, 0x0F)
    assert ((status & 0x0F) != 0).sum() > 10 and ((status != 0) & ((status & 0x0F) == 0)).sum() > 10
    assert (status == 0).sum() > 100


# ----------------------------------------------------------------------------------- accuracy
# The largest |nu - generating nu| in natural bins (1 / channels), over ACCURACY_TONES random
# noise-free unit tones per shape whose samples are rounded to float32, measured on the host
# class; the tests assert twice these. From a start of up to an eighth of a natural bin away
# three steps already leave nothing of Newton's own residual: 3 and 6 steps end at the same
# error, which is what the float32 rounding of the samples does to the likelihood's maximum.
ACCURACY_SHAPES = [(64, 256), (1000, 4096), (4096, 16384)]
ACCURACY_TONES = 64
MEASURED_NOISE_FREE = {
    (64, 256, 3): 2.185e-9, (64, 256, 6): 2.185e-9,
    (1000, 4096, 3): 5.232e-10, (1000, 4096, 6): 5.232e-10,
    (4096, 16384, 3): 3.092e-10, (4096, 16384, 6): 3.092e-10,
}  # fmt: skip
# With amplitude scatter of 30 %, noise of 0.3 per channel and a tenth of the channels missing:
# the largest |nu - reference nu| in natural bins and the largest |phasor - reference phasor|
# against inputs_fit_delays.reference_fit (float64, np.fft, Newton until it stands), refine=6.
# Both compute in float64, so the first is their rounding; the second is the float32 rounding
# of the phasor.
MEASURED_NOISY_NU = {(64, 256): 2.256e-13, (1000, 4096): 1.110e-13, (4096, 16384): 4.547e-13}
MEASURED_NOISY_PHASOR = {(64, 256): 3.983e-8, (1000, 4096): 3.282e-8, (4096, 16384): 3.428e-8}


def wrapped(difference):
    return np.abs(difference - np.rint(difference))


def noise_free_error(channels, n_fft, refine):
    rs = np.random.RandomState(channels)
    nus = rs.uniform(-0.5, 0.5, ACCURACY_TONES)
    phases = rs.uniform(-np.pi, np.pi, ACCURACY_TONES)
    c = np.arange(channels)[:, np.newaxis]
    gains = np.exp(1j * (phases + 2 * np.pi * c * nus)).astype(np.complex64)
    delays, _, amplitudes, fit_status, _ = host.FitDelaysHost(1.0, n_fft, refine)(gains)
    assert not fit_status.any() and np.abs(amplitudes - 1).max() < 1e-3
    return wrapped(delays - nus).max() * channels


def noisy_errors(channels, n_fft):
    gains, _, _ = gen.make_gains(channels, channels, ACCURACY_TONES, n_fft,
                                 kinds=("noisy", "missing"))  # fmt: skip
    delays, phasors, amplitudes, fit_status, _ = host.FitDelaysHost(1.0, n_fft, 6)(gains)
    assert not fit_status.any()
    nu, phasor, amplitude = gen.reference_fit(gains, n_fft)
    assert np.abs(amplitudes / amplitude - 1).max() < 1e-5
    return wrapped(delays - nu).max() * channels, np.abs(phasors - phasor).max()


@pytest.mark.parametrize("refine", [3, 6])
@pytest.mark.parametrize("channels, n_fft", ACCURACY_SHAPES)
def test_accuracy_noise_free(channels, n_fft, refine):
    error = noise_free_error(channels, n_fft, refine)
    print(f"noise-free {channels}/{n_fft} refine {refine}: {error:.3e} natural bins")
    assert error <= 2 * MEASURED_NOISE_FREE[channels, n_fft, refine]


@pytest.mark.parametrize("channels, n_fft", ACCURACY_SHAPES)
def test_accuracy_with_noise(channels, n_fft):
    nu_error, phasor_error = noisy_errors(channels, n_fft)
    print(f"noisy {channels}/{n_fft}: {nu_error:.3e} natural bins, phasor {phasor_error:.3e}")
    assert nu_error <= 2 * MEASURED_NOISY_NU[channels, n_fft]
    assert phasor_error <= 2 * MEASURED_NOISY_PHASOR[channels, n_fft]


# ----------------------------------------------------------------------------------- recovery
# The largest |calibrated cross-correlation - 1| over the samples that are not flagged, measured
# on the host classes; the test asserts twice this. Without the fit (gains of 1) it is about 2.
MEASURED_RECOVERY = 4.248e-3


def recovery_case():
    """vis, weights, flags and inputs of a unit source seen through 12 inputs with delays of up
    to 0.01 turns per channel and phases of their own, with noise of 1e-3, 128 channels."""
    channels, n_inputs = 128, 12
    rs = np.random.RandomState(77)
    ants = np.ascontiguousarray(np.array(np.triu_indices(n_inputs, 1)).T, np.int32)
    nus = rs.uniform(-0.01, 0.01, n_inputs)
    phases = rs.uniform(-np.pi, np.pi, n_inputs)
    c = np.arange(channels)[:, np.newaxis]
    truth = np.exp(1j * (phases + 2 * np.pi * c * nus))
    shape = (channels, len(ants))
    noise = 1e-3 * (rs.standard_normal(shape) + 1j * rs.standard_normal(shape))
    vis = (truth[:, ants[:, 0]] * np.conj(truth[:, ants[:, 1]]) + noise).astype(np.complex64)
    weights = np.ones(shape, f32)
    flags = np.zeros(shape, np.uint8)
    # the solver loses a tenth of the channels altogether
    lost = rs.random_sample(channels) < 0.1
    flags[lost] = 1
    return vis, weights, flags, ants, nus, lost


def recovery_error():
    vis, weights, flags, ants, nus, lost = recovery_case()
    pairs = host.SolveGainsHost.pair_table(ants, 12)
    gains, _, status = host.SolveGainsHost()(vis, pairs, weights, flags)
    assert np.isnan(gains[lost].real).all() and (status[lost] != 0).all() and lost.sum() > 5
    delays, _, amplitudes, fit_status, model = host.FitDelaysHost(1.0, corrections=True)(gains, status)
    assert not fit_status.any() and np.abs(amplitudes - 1).max() < 1e-2
    assert np.abs((delays - delays[0]) - (nus - nus[0])).max() < 1e-6
    # the corrections cover the channels the solver lost too
    cal_vis, _, cal_flags = host.ApplyGainsHost()(vis, model, ants, weights, np.zeros_like(flags))
    assert not cal_flags.any()
    raw = np.abs(vis - 1).max()
    return np.abs(cal_vis - 1).max(), raw


def test_recovers_the_unit_source():
    error, raw = recovery_error()
    print(f"recovery: {error:.3e} (uncalibrated {raw:.3f})")
    assert error <= 2 * MEASURED_RECOVERY and raw > 1.5


# ----------------------------------------------------------------------------------- errors
def test_host_errors():
    for bad in (0, 0.0, np.inf, -np.inf, np.nan, "wide", None):
        with pytest.raises(ValueError, match="channel_width"):
            host.FitDelaysHost(bad)
    for bad in (0, 2, 3, 6, 100, 32768, -4):
        with pytest.raises(ValueError, match="n_fft"):
            host.FitDelaysHost(1e6, bad)
    for bad in (4.0, True, "8"):
        with pytest.raises(TypeError, match="n_fft"):
            host.FitDelaysHost(1e6, bad)
    for bad in (-1, 9):
        with pytest.raises(ValueError, match="refine"):
            host.FitDelaysHost(1e6, refine=bad)
    for bad in (1.0, False):
        with pytest.raises(TypeError, match="refine"):
            host.FitDelaysHost(1e6, refine=bad)
    for bad in (-1, 256):
        with pytest.raises(ValueError, match="status_mask"):
            host.FitDelaysHost(1e6, status_mask=bad)
    with pytest.raises(TypeError, match="status_mask"):
        host.FitDelaysHost(1e6, status_mask=1.0)
    fn = host.FitDelaysHost(-1e6)
    assert (fn.channel_width, fn.n_fft, fn.refine, fn.status_mask, fn.corrections) == (
        -1e6, None, 3, 255, False)  # fmt: skip
    assert [fn.transform_length(c) for c in (1, 2, 3, 64, 65, 4096, 4097, 8192)] == [
        4, 8, 16, 256, 512, 16384, 16384, 16384]  # fmt: skip
    assert host.FitDelaysHost(1.0, 4).transform_length(2) == 4
    assert host.FitDelaysHost(1.0, np.int64(16384), np.int32(8)).transform_length(8192) == 16384
    for channels, n_fft in ((3, 4), (65, 128), (8192, 8192)):
        with pytest.raises(ValueError, match="n_fft"):
            host.FitDelaysHost(1.0, n_fft).transform_length(channels)
    for bad in (0, -1, 8193):
        with pytest.raises(ValueError, match="channels"):
            fn.transform_length(bad)
    with pytest.raises(ValueError, match="n_inputs"):
        fn.transform_length(4, 0)
    good = gen.make_gains(1, 6, 3, 32)[0]
    status = np.zeros(6, np.uint8)
    fn(good, status)
    for bad in (good.astype(np.complex128), good[0], good[:0], good[:, :0], good.real,
                np.zeros((8193, 1), np.complex64)):  # fmt: skip
        with pytest.raises(ValueError, match="gains"):
            fn(bad, status)
    for bad in (status.astype(np.int8), status[:5], status[:, np.newaxis], np.zeros(7, np.uint8)):
        with pytest.raises(ValueError, match="status"):
            fn(good, bad)
    with pytest.raises(ValueError, match="n_fft"):
        host.FitDelaysHost(1.0, 8)(good)
    assert (host.FitDelaysHost.MIN_FFT, host.FitDelaysHost.MAX_FFT, host.FitDelaysHost.MAX_CHANNELS,
            host.FitDelaysHost.MAX_REFINE) == (4, 16384, 8192, 8)  # fmt: skip
    assert (host.FitDelaysHost.NO_FIT, host.FitDelaysHost.STEP_REJECTED) == (NO_FIT, STEP_REJECTED)


def test_template_and_operation_errors(context, queue):
    with pytest.raises(ValueError):
        ingest.FitDelaysTemplate(context, 1e6, tuning={"wgs": 256})
    assert ingest.FitDelaysTemplate(context, 1e6, tuning={}).tuning == {}
    assert ingest.FitDelaysTemplate.autotune(context) == {}
    assert ingest.FitDelaysTemplate.TUNING_KEYS == ()
    assert ingest.FitDelaysTemplate.host_class is host.FitDelaysHost
    assert ingest.FitDelaysTemplate.KERNEL == "ksp_fit_delays"
    assert ingest.FitDelaysTemplate.operation_class is ingest.FitDelays
    for name, bads in (("channel_width", (0, np.nan, np.inf)), ("n_fft", (0, 6, 32768)),
                       ("refine", (-1, 9)), ("status_mask", (-1, 256))):  # fmt: skip
        for bad in bads:
            with pytest.raises(ValueError, match=name):
                ingest.FitDelaysTemplate(context, **{"channel_width": 1e6, name: bad})
    for name in ("n_fft", "refine", "status_mask"):
        with pytest.raises(TypeError, match=name):
            ingest.FitDelaysTemplate(context, **{"channel_width": 1e6, name: 1.5})
    template = ingest.FitDelaysTemplate(context, 1e6)
    assert template.kernel.name == "ksp_fit_delays"
    assert (template.channel_width, template.n_fft, template.refine, template.status,
            template.status_mask, template.model, template.corrections) == (
        1e6, None, 3, True, 255, True, False)  # fmt: skip
    for args in [(0, 4), (-1, 4), (8193, 4), (4, 0), (4, -1)]:
        with pytest.raises(ValueError):
            template.instantiate(queue, *args)
    assert isinstance(template.instantiate(queue, 8192, 1), ingest.FitDelays)
    fixed = ingest.FitDelaysTemplate(context, 1e6, n_fft=64)
    assert fixed.instantiate(queue, 32, 5).n_fft == 64
    with pytest.raises(ValueError, match="n_fft"):
        fixed.instantiate(queue, 33, 5)
    fn = ingest.FitDelaysTemplate(context, -2e5, None, 5, False, 0x30, False, True).instantiate(
        queue, 100, 7)  # fmt: skip
    assert fn.parameters() == {"channel_width": -2e5, "n_fft": 512, "refine": 5, "status": False,
                               "status_mask": 0x30, "model": False, "corrections": True,
                               "channels": 100, "n_inputs": 7}  # fmt: skip


def test_host_from_device(context, queue):
    gains = gen.make_gains(1, 10, 5, 64)[0]
    status = np.zeros(10, np.uint8)
    for with_status, with_model, corrections in VARIANTS:
        template = ingest.FitDelaysTemplate(context, 1e6, None, 3, with_status, 0xFF, with_model,
                                            corrections)  # fmt: skip
        adapter = ingest.FitDelaysHostFromDevice(template, queue)
        del queue.launches[:]
        out = adapter(gains, status if with_status else None)
        assert len(out) == 5 and (out[4] is not None) == with_model
        for o, shape, dtype in zip(out, [(5,)] * 4 + [(10, 5)],
                                   (f64, np.complex64, f32, np.uint8, np.complex64)):  # fmt: skip
            assert o is None or (o.shape, o.dtype) == (shape, dtype)
        assert [name for name, _ in queue.launches] == ["ksp_fit_delays"]
        assert [int(a) for a in queue.launches[0][1][7:9]] == [10, 5]
        with pytest.raises(TypeError, match="status"):
            adapter(gains, None if with_status else status)
    adapter = ingest.FitDelaysHostFromDevice(ingest.FitDelaysTemplate(context, 1e6, 8, status=False), queue)
    with pytest.raises(ValueError, match="n_fft"):
        adapter(gains)
    with pytest.raises(ValueError):
        adapter(gains[:0])


# ----------------------------------------------------------------------------------- wiring
@pytest.mark.parametrize("with_status, with_model, corrections", VARIANTS)
def test_slots_and_launch_arguments(with_status, with_model, corrections, context, queue):
    template = ingest.FitDelaysTemplate(context, -7.5e5, 2048, 4, with_status, 0x3C, with_model,
                                        corrections)  # fmt: skip
    fn = template.instantiate(queue, 300, 58)
    names = ["gains"] + (["status"] if with_status else []) + [
        "delays", "phasors", "amplitudes", "fit_status"] + (["model"] if with_model else [])  # fmt: skip
    assert list(fn.slots) == names
    shapes = {"gains": ((300, 58), np.complex64), "status": ((300,), np.uint8),
              "delays": ((58,), f64), "phasors": ((58,), np.complex64),
              "amplitudes": ((58,), f32), "fit_status": ((58,), np.uint8),
              "model": ((300, 58), np.complex64)}  # fmt: skip
    for name, slot in fn.slots.items():
        assert (slot.shape, slot.dtype) == shapes[name], name
    # a dimension object of its own for everything that can be padded
    dims = [d for slot in fn.slots.values() for d in slot.dimensions]
    assert len({id(d) for d in dims}) == len(dims) == len(fn.slots) + 1 + with_model
    accel.Dimension(58, min_padded_size=100).link(fn.slots["gains"].dimensions[1])
    if with_model:
        accel.Dimension(58, min_padded_size=200).link(fn.slots["model"].dimensions[1])
    fn()
    assert [name for name, _ in queue.launches] == ["ksp_fit_delays"]
    args = queue.launches[0][1]
    assert len(args) == 16
    order = ["gains", "status", "delays", "phasors", "amplitudes", "fit_status", "model"]
    for got, name in zip(args[:7], order):
        assert got is (fn.buffer(name).buffer if name in names else None), name
    assert all(isinstance(a, np.int32) for a in args[7:15]) and isinstance(args[15], f64)
    assert [int(a) for a in args[7:9]] == [300, 58]
    assert int(args[9]) == fn.buffer("gains").padded_shape[1] == 112  # whole 128-byte rows
    assert int(args[10]) == (fn.buffer("model").padded_shape[1] if with_model else 0)
    assert int(args[10]) == (208 if with_model else 0)
    assert [int(a) for a in args[11:15]] == [2048, 4, 0x3C, int(corrections)]
    assert float(args[15]) == -7.5e5


def test_default_transform_length_is_a_launch_argument(context, queue):
    template = ingest.FitDelaysTemplate(context, 1e6)
    for channels, n_fft in ((1, 4), (2, 8), (1000, 4096), (1025, 8192), (8192, 16384)):
        del queue.launches[:]
        template.instantiate(queue, channels, 3)()
        assert int(queue.launches[0][1][11]) == n_fft


def test_between_solve_and_apply(context, queue):
    """solve_gains -> fit_delays -> apply_gains: fit reads the solver's gains and status, and
    apply_gains multiplies by fit's model; each pair takes the larger padding of the two."""
    rows, baselines, n_inputs = 64, 66, 12
    solve = ingest.SolveGainsTemplate(context).instantiate(queue, rows, baselines, n_inputs)
    fit = ingest.FitDelaysTemplate(context, 1e6, corrections=True).instantiate(queue, rows, n_inputs)
    apply_gains = ingest.ApplyGainsTemplate(context).instantiate(queue, rows, baselines, n_inputs)
    accel.Dimension(n_inputs, min_padded_size=40).link(solve.slots["gains"].dimensions[1])
    accel.Dimension(n_inputs, min_padded_size=70).link(apply_gains.slots["gains"].dimensions[1])
    accel.Dimension(rows, min_padded_size=100).link(fit.slots["status"].dimensions[0])
    seq = accel.OperationSequence(
        queue, [("solve", solve), ("fit", fit), ("apply_gains", apply_gains)],
        compounds={"vis": ["solve:vis", "apply_gains:vis"],
                   "weights": ["solve:weights", "apply_gains:weights"],
                   "flags": ["solve:flags", "apply_gains:flags"],
                   "gains": ["solve:gains", "fit:gains"],
                   "status": ["solve:status", "fit:status"],
                   "corrections": ["fit:model", "apply_gains:gains"]})  # fmt: skip
    assert {"vis", "weights", "flags", "gains", "status", "corrections", "solve:pairs",
            "solve:iterations", "fit:delays", "fit:phasors", "fit:amplitudes", "fit:fit_status",
            "apply_gains:inputs", "apply_gains:out_vis"} <= set(seq.slots)  # fmt: skip
    seq()
    assert [name for name, _ in queue.launches] == [
        "ksp_solve_gains", "ksp_fit_delays", "ksp_apply_gains"]  # fmt: skip
    solve_args, fit_args, apply_args = (launch[1] for launch in queue.launches)
    assert solve_args[5] is fit_args[0] is seq.buffer("gains").buffer
    assert solve_args[7] is fit_args[1] is seq.buffer("status").buffer
    assert fit_args[6] is apply_args[3] is seq.buffer("corrections").buffer
    assert seq.buffer("gains").buffer is not seq.buffer("corrections").buffer
    assert int(solve_args[16]) == int(fit_args[9]) == seq.buffer("gains").padded_shape[1] == 48
    assert int(fit_args[10]) == int(apply_args[14]) == 80
    assert seq.buffer("status").padded_shape[0] >= 100
    assert [int(a) for a in fit_args[7:9]] == [rows, n_inputs] and int(fit_args[11]) == 256


# ------------------------------------------------------------------- the launcher's checks
@pytest.fixture(scope="module")
def lib():
    from katsdpsigproc_amd import _lib, build_native

    if not os.path.exists(_lib.LIB_PATH):
        build_native.build()
    return _lib.load()


POINTERS = ["gains", "status", "delays", "phasors", "amplitudes", "fit_status", "model"]
NUMBERS = ["channels", "n_inputs", "gains_stride", "model_stride", "n_fft", "refine",
           "status_mask", "corrections"]  # fmt: skip


def test_argument_validation_without_gpu(lib):
    from katsdpsigproc_amd import _lib

    # never dereferenced: every call below fails its checks first. Seven arrays far apart.
    p = {name: ctypes.c_void_p((i + 1) << 32) for i, name in enumerate(POINTERS)}
    good = dict(channels=4, n_inputs=8, gains_stride=8, model_stride=8, n_fft=16, refine=3,
                status_mask=255, corrections=0, channel_width=1e6)  # fmt: skip

    def call(device=0, **changed):
        a = dict(p, **good)
        a.update(changed)
        rc = lib.ksp_fit_delays(device, None, *(a[name] for name in POINTERS),
                                *(a[name] for name in NUMBERS), a["channel_width"])  # fmt: skip
        assert rc != 0
        return _lib.last_error()

    for name in ("gains", "delays", "phasors", "amplitudes", "fit_status"):
        assert f"invalid argument: {name} is NULL" in call(**{name: None})
    for bad in (0, -1, 8193):
        assert "invalid argument: channels must be 1..8192" in call(channels=bad, n_fft=16384)
    for bad in (0, -1):
        assert "invalid argument: n_inputs must be at least 1" in call(n_inputs=bad)
    for bad in (0, 2, 3, 12, -16, 32768):
        assert "invalid argument: n_fft must be a power of two in 4..16384" in call(n_fft=bad)
    assert "invalid argument: n_fft must be at least twice the channels" in call(n_fft=4)
    assert "n_fft must be at least twice" in call(channels=8192, n_fft=8192)
    for bad in (-1, 9):
        assert "invalid argument: refine must be 0..8" in call(refine=bad)
    for bad in (-1, 256):
        assert "invalid argument: status_mask must be 0..255" in call(status_mask=bad)
    for bad in (-1, 2):
        assert "invalid argument: corrections must be 0 or 1" in call(corrections=bad)
    for bad in (0.0, -0.0, float("inf"), float("-inf"), float("nan")):
        assert "invalid argument: channel_width must be finite and not 0" in call(channel_width=bad)
    for name in ("gains", "model"):
        assert f"invalid argument: {name}_stride is smaller than n_inputs" in call(
            **{name + "_stride": 7})
    # the order of the checks: everything wrong at once, then one thing fewer at a time
    wrong = dict(channels=0, n_inputs=0, gains_stride=-1, model_stride=-1, n_fft=0, refine=-1,
                 status_mask=-1, corrections=2, channel_width=0.0)  # fmt: skip
    assert "invalid argument: gains is NULL" in call(**dict.fromkeys(p), **wrong)
    order = [("channels", "channels must be"), ("n_inputs", "n_inputs must be"),
             ("n_fft", "n_fft must be a power"), ("refine", "refine must be"),
             ("status_mask", "status_mask must be"), ("corrections", "corrections must be"),
             ("channel_width", "channel_width must be"), ("gains_stride", "gains_stride is smaller"),
             ("model_stride", "model_stride is smaller")]  # fmt: skip
    for name, message in order:
        assert message in call(**wrong), name
        wrong[name] = good[name]
    # an absent array's stride is not looked at, and status may be absent
    assert "hipSetDevice(device) failed" in call(device=-1, model=None, model_stride=-1)
    assert "hipSetDevice(device) failed" in call(device=-1, status=None)

    # model shares no byte with gains, not even as the same array
    def at(name, offset):
        return ctypes.c_void_p(p[name].value + offset)

    extent = (3 * 8 + 8) * 8  # the bytes from the first element to the last
    assert "invalid argument: model overlaps gains" in call(model=p["gains"])
    assert "invalid argument: model overlaps gains" in call(model=at("gains", extent - 1))
    assert "invalid argument: model overlaps gains" in call(model=at("gains", -(extent - 1)))
    # arrays that only touch pass every check: what is left to fail is the first device call,
    # which device -1 fails on any machine
    for touching in (dict(model=at("gains", extent)), dict(model=at("gains", -extent)),
                     dict(channels=8192, n_fft=16384), dict(channels=1, n_fft=4, refine=0)):  # fmt: skip
        assert "hipSetDevice(device) failed" in call(device=-1, **touching)


def test_header_binding_and_exports_agree(lib):
    from katsdpsigproc_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "katsdpsigproc_hip.h")).read()
    comment = re.search(r"/\* fit_delays:.*?\*/", text, re.S).group(0)
    assert "FitDelaysHost" in comment
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declaration = re.search(r"int ksp_fit_delays\((.*?)\);", text, re.S)
    assert declaration is not None
    parameters = [" ".join(part.split()) for part in declaration.group(1).split(",")]
    argtypes = _lib.SIGNATURES["ksp_fit_delays"]
    assert len(parameters) == len(argtypes) == 18
    for parameter, argtype in zip(parameters, argtypes):
        assert ("*" in parameter) == (argtype is ctypes.c_void_p), parameter
        by_value = parameter.startswith("double ") and "*" not in parameter
        assert by_value == (argtype is ctypes.c_double), parameter
        assert argtype in (ctypes.c_int, ctypes.c_void_p, ctypes.c_double)
    names = [parameter.replace("*", " ").split()[-1] for parameter in parameters]
    assert names == ["device", "stream"] + POINTERS + NUMBERS + ["channel_width"]
    assert hasattr(lib, "ksp_fit_delays") and "ksp_fit_delays" in _lib.declared_symbols()
    assert lib.ksp_abi_version() == _lib.ABI_VERSION == 5
    for name in ("FitDelaysTemplate", "FitDelays", "FitDelaysHostFromDevice"):
        assert hasattr(ingest, name)
    assert hasattr(host, "FitDelaysHost")
    # the header comment, the host class and the kernel show the same digits; the series is the
    # one copy that the kernel includes, and the kernel has none of its own
    csrc = os.path.join(root, "katsdpsigproc_amd", "csrc")
    series = open(os.path.join(csrc, "cal_math.h")).read()
    kernel = open(os.path.join(csrc, "fit_delays.hip")).read()
    assert repr(host.FitDelaysHost.TWO_PI) in comment and repr(host.FitDelaysHost.TWO_PI) in kernel
    assert '#include "cal_math.h"' in kernel and "ksp_cos_sin_turns(" in kernel
    for value in host.PredictHost.SIN_COEFFICIENTS + host.PredictHost.COS_COEFFICIENTS:
        assert series.count(repr(abs(value))) >= 2, value
        if abs(value) not in (1.0, 0.5):  # (digits that text has for other reasons)
            assert repr(abs(value)) not in kernel, value
