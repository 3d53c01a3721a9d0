"""Predicting model visibilities without a GPU: ``rfi.host.PredictHost`` against a loop of
Python floats and float32 scalars, against a longdouble evaluation, on exact phases and on the
samples that have no usable model; the model in front of ``SolveGainsHost``; argument errors,
slot lists and every launch argument of every variant on the fake backend, the sequence
finalise -> predict -> solve -> apply_gains, and the argument checks of ``ksp_predict``, which
come before any device call."""

import ctypes
import math
import os
import re

import numpy as np
import pytest

from katsdpsigproc_amd import accel
from katsdpsigproc_amd.rfi import device, host, ingest
from tests import inputs_predict as gen
from tests import inputs_solve_gains as gen_solve
from tests.fakes import FakeContext
from tests.inputs_predict import assert_same

f32 = np.float32
#: (model, divide, weights, flags) of every kernel variant
VARIANTS = [(True, False, False, False)] + [
    (model, True, weights, flags)
    for model in (True, False) for weights in (True, False) for flags in (True, False)]  # fmt: skip
SQRT_HALF = math.sqrt(0.5)


@pytest.fixture
def context():
    return FakeContext()


@pytest.fixture
def queue(context):
    return context.create_command_queue()


# ----------------------------------------------------------------------------- the scalar loop
def rint(x):
    """To nearest, ties to even, on a Python float (round() does the ties; it loses the sign of
    a zero and refuses what is not finite)."""
    if x != x or abs(x) >= 2.0**52:
        return x
    return math.copysign(float(round(x)), x)


def scalar_cos_sin(x):
    s, c = host.PredictHost.SIN_COEFFICIENTS, host.PredictHost.COS_COEFFICIENTS
    r = x - rint(x)
    q = rint(4.0 * r)
    y = r - q * 0.25
    z = y * 6.283185307179586
    z2 = z * z
    sn = (((((s[5] * z2 + s[4]) * z2 + s[3]) * z2 + s[2]) * z2 + s[1]) * z2 + s[0]) * z
    cs = (((((c[6] * z2 + c[5]) * z2 + c[4]) * z2 + c[3]) * z2 + c[2]) * z2 + c[1]) * z2 + c[0]
    k = int(q) & 3 if q == q else 0
    return [(cs, sn), (-sn, cs), (-cs, -sn), (sn, -cs)][k]


def scalar_loop(freqs, delays, flux, vis, weights, flags, flag_value):
    """The definition, sample by sample and step by step: Python floats for the model (every
    operator one float64 operation), np.float32 scalars for the division."""
    channels, (n_sources, baselines) = len(freqs), delays.shape
    model = np.empty((channels, baselines), np.complex64)
    out_vis, out_weights, out_flags = np.empty_like(vis), np.empty_like(weights), np.empty_like(flags)
    with np.errstate(all="ignore"):
        for c in range(channels):
            for j in range(baselines):
                acc_re = acc_im = 0.0
                for s in range(n_sources):
                    co, si = scalar_cos_sin(float(freqs[c]) * float(delays[s, j]))
                    amplitude = float(flux[c, s])
                    acc_re = acc_re + amplitude * co
                    acc_im = acc_im - amplitude * si
                mr, mi = f32(acc_re), f32(acc_im)
                model[c, j] = complex(mr, mi)
                d = f32(f32(mr * mr) + f32(mi * mi))
                vr, vi = f32(vis[c, j].real), f32(vis[c, j].imag)
                if d > 0 and d < np.inf:
                    out_vis[c, j] = complex(f32(f32(f32(vr * mr) + f32(vi * mi)) / d),
                                            f32(f32(f32(vi * mr) - f32(vr * mi)) / d))  # fmt: skip
                    out_weights[c, j] = f32(weights[c, j] * d)
                    out_flags[c, j] = flags[c, j]
                else:
                    out_vis[c, j] = vis[c, j]
                    out_weights[c, j] = 0
                    out_flags[c, j] = flags[c, j] | flag_value
    return model, out_vis, out_weights, out_flags


NAMES = ("model", "out_vis", "out_weights", "out_flags")


@pytest.mark.parametrize("channels, baselines, n_sources, pattern, flag_value", [
    (5, 23, 3, "random", 64), (3, 17, 7, "large", 1), (8, 40, 2, "exact", 255),
    (3, 30, 4, "huge", 64), (6, 25, 5, "nonfinite", 16), (5, 20, 6, "flux", 64),
    (3, 9, 5, "cancel", 128), (1, 1, 1, "random", 64), (2, 3, 64, "random", 64)])  # fmt: skip
def test_host_against_scalar_loop(channels, baselines, n_sources, pattern, flag_value):
    case = gen.make_case(10 * channels + baselines, channels, baselines, n_sources, pattern,
                         flag_value)  # fmt: skip
    before = {name: value.copy() for name, value in case.items()}
    fn = host.PredictHost(flag_value)
    got = fn(**case)
    want = scalar_loop(flag_value=flag_value, **case)
    for name, w, g in zip(NAMES, want, got):
        assert_same(w, g, name)
        assert g.flags.c_contiguous
    for name, value in case.items():  # the inputs are never modified
        assert_same(before[name], value, name)
    # each optional array on its own, and none, give the same answers
    model_args = (case["freqs"], case["delays"], case["flux"])
    only_model = fn(*model_args)
    assert only_model[1:] == (None, None, None)
    only_w = fn(*model_args, case["vis"], weights=case["weights"])
    only_f = fn(*model_args, case["vis"], flags=case["flags"])
    neither = fn(*model_args, case["vis"])
    assert only_w[3] is None and only_f[2] is None and neither[2] is None and neither[3] is None
    for other in (only_model, only_w, only_f, neither):
        assert_same(got[0], other[0], "model")
    for other in (only_w, only_f, neither):
        assert_same(got[1], other[1], "out_vis")
    assert_same(got[2], only_w[2], "out_weights")
    assert_same(got[3], only_f[3], "out_flags")


def test_generators_cover_the_cases():
    exact = gen.make_model(1, 8, 400, 3, "exact")
    x = exact["freqs"][:, np.newaxis, np.newaxis] * exact["delays"][np.newaxis]
    r = x - np.rint(x)
    assert set(np.unique(np.abs(r))) == {0, 0.125, 0.25, 0.375, 0.5}
    assert (r == 0.5).any() and (r == -0.5).any()  # ties of the first rint, both ways
    assert (np.abs(4 * r) == 0.5).any() and (np.abs(4 * r) == 1.5).any()  # and of the second
    assert np.signbit(exact["delays"][exact["delays"] == 0]).any()
    huge = gen.make_model(1, 3, 400, 3, "huge")
    x = huge["freqs"][:, np.newaxis, np.newaxis] * huge["delays"][np.newaxis]
    assert (np.abs(x) >= 2.0**52).mean() > 0.5 and (np.abs(x - np.rint(x)) == 0.5).any()
    assert (np.abs(x[np.abs(x) >= 2.0**52] - np.rint(x[np.abs(x) >= 2.0**52])) == 0).all()
    large = gen.make_model(1, 5, 400, 3, "large")
    assert np.abs(large["freqs"][:, np.newaxis, np.newaxis] * large["delays"]).max() > 2.0**19.9
    bad = gen.make_model(1, 40, 400, 30, "nonfinite")
    for name in ("freqs", "delays", "flux"):
        assert np.isnan(bad[name]).any() and np.isposinf(bad[name]).any() \
            and np.isneginf(bad[name]).any(), name  # fmt: skip
    flux = gen.make_model(1, 40, 10, 30, "flux")["flux"]
    for value in gen.SPECIAL_FLUX:
        assert (flux.view(np.uint32) == f32(value).view(np.uint32)).any()
    assert not flux[0].any() and (flux[1] == f32(1e-30)).all() and (flux[2] == f32(3e38)).all()
    for n_sources in (1, 2, 5):
        cancel = gen.make_model(1, 4, 10, n_sources, "cancel")
        assert not host.PredictHost()(**cancel)[0].any()
    for pattern in gen.PATTERNS:
        made = gen.make_case(1, 3, 17, 5, pattern)
        assert [made[name].dtype for name in ("freqs", "delays", "flux", "vis", "weights", "flags")] \
            == [np.float64, np.float64, f32, np.complex64, f32, np.uint8]  # fmt: skip
        assert made["delays"].shape == (5, 17) and made["flux"].shape == (3, 5)
        assert all(value.flags.c_contiguous for value in made.values())


# ------------------------------------------------------------------------------- accuracy
@pytest.mark.parametrize("n_sources", [1, 3, 64])
def test_accuracy_against_longdouble(n_sources):
    """Up to 2^20 turns, fluxes of both signs: |model - reference| <= 2^-23 sum_s |flux[c, s]|,
    half an ulp of float32 on a value of at most sum |flux|, doubled; the float64 terms (7e-12
    per source from the series, 2^-53 per operation) are below 1e-9 of it."""
    worst = 0.0
    for seed in (1, 2, 3):
        case = gen.make_model(seed, 6, 300, n_sources, "large")
        assert (case["flux"] > 0).any() and (case["flux"] < 0).any()
        model = host.PredictHost()(**case)[0]
        reference = gen.reference_model(**case)
        error = np.abs(model.astype(np.clongdouble) - reference)
        bound = 2.0**-23 * np.abs(case["flux"].astype(np.float64)).sum(axis=1)[:, np.newaxis]
        worst = max(worst, float((error / bound).max()))
        assert (error <= bound).all()
    print(f"largest |model - reference| over the bound with {n_sources} sources: {worst:.3f}")


def test_series_error():
    """(co, si) against longdouble on phases up to 2 10^5 turns: 7e-12 measured."""
    rs = np.random.RandomState(4)
    x = rs.uniform(-2e5, 2e5, 200000)
    co, si = host.PredictHost.cos_sin(x)
    angle = 8 * np.arctan(np.longdouble(1)) * (x - np.rint(x)).astype(np.longdouble)
    worst = max(np.abs(co - np.cos(angle)).max(), np.abs(si - np.sin(angle)).max())
    print(f"largest error of (co, si): {float(worst):.2e}")
    assert worst < 1e-11


# ------------------------------------------------------------------------------ exact cases
def bits(values):
    return np.asarray(values, np.float64).view(np.uint64).tolist()


#: x, co, si: the sign of every zero included
EXACT = [
    (0.0, 1.0, 0.0), (-0.0, 1.0, 0.0), (1.0, 1.0, 0.0), (-3.0, 1.0, 0.0),
    (0.25, -0.0, 1.0), (-0.25, 0.0, -1.0), (0.75, 0.0, -1.0), (-0.75, -0.0, 1.0),
    (0.5, -1.0, -0.0), (-0.5, -1.0, -0.0), (1.5, -1.0, -0.0), (2.5, -1.0, -0.0), (-1.5, -1.0, -0.0),
    (2.0**52, 1.0, 0.0), (-(2.0**52), 1.0, 0.0), (2.0**52 + 1, 1.0, 0.0), (2.0**60, 1.0, 0.0),
    (-(2.0**200), 1.0, 0.0), (2.0**51 + 0.5, -1.0, -0.0), (2.0**51 + 1.5, -1.0, -0.0),
    (-(2.0**51) - 0.5, -1.0, -0.0), (2.0**50 + 0.25, -0.0, 1.0), (2.0**50 - 0.25, 0.0, -1.0),
]  # fmt: skip


def test_exact_phases():
    x = np.array([row[0] for row in EXACT])
    co, si = host.PredictHost.cos_sin(x)
    assert bits(co) == bits([row[1] for row in EXACT])
    assert bits(si) == bits([row[2] for row in EXACT])
    for value, c, s in zip(x, co, si):
        assert bits(scalar_cos_sin(float(value))) == bits([c, s])
    # r = x - rint(x) on the halves: to even, so 0.5 stays +0.5 and 1.5 becomes -0.5
    assert (x[8:13] - np.rint(x[8:13])).tolist() == [0.5, -0.5, -0.5, 0.5, 0.5]
    # the eighths: q = rint(4 r) rounds +-0.5 to 0 and +-1.5 to +-2, and |z| = pi/4 either way
    eighths = (2 * np.arange(-8, 9) + 1) / 8.0
    co, si = host.PredictHost.cos_sin(eighths)
    want = np.exp(2j * np.pi * eighths)
    assert np.abs(co - want.real).max() < 1e-11 and np.abs(si - want.imag).max() < 1e-11
    assert np.abs(np.abs(co) - SQRT_HALF).max() < 1e-11
    # non-finite turns are NaN in both
    co, si = host.PredictHost.cos_sin(np.array([np.inf, -np.inf, np.nan]))
    assert np.isnan(co).all() and np.isnan(si).all()


def test_exact_model():
    """Through __call__ with powers of two: x = freqs * delays is exact, the model is +-1 or
    +-i with the zero the definition gives: re = +0 + F co, im = +0 - F si."""
    freqs = np.array([1.0, 2.0, 4.0])
    delays = np.array([[0.0, 0.125, 0.25, 0.375, 0.5, -0.125, 2.0**52, 2.0**49 + 0.125]])
    model = host.PredictHost()(freqs, delays, np.ones((3, 1), f32))[0]
    assert model.dtype == np.complex64
    x = freqs[:, np.newaxis] * delays
    co, si = host.PredictHost.cos_sin(x)
    assert_same((0.0 + co).astype(f32), np.ascontiguousarray(model.real), "re")
    assert_same((0.0 - si).astype(f32), np.ascontiguousarray(model.imag), "im")
    assert model[0].tolist()[:5] == [1, complex(f32(SQRT_HALF), -f32(SQRT_HALF)), -1j,
                                     complex(-f32(SQRT_HALF), -f32(SQRT_HALF)), -1]  # fmt: skip
    assert model[1].tolist()[:5] == [1, -1j, -1, 1j, 1]
    assert model[2].tolist() == [1, -1, 1, -1, 1, -1, 1, -1]
    assert not np.signbit(model[2].imag[[0, 2, 4, 6]]).any()  # +0 - (+0)
    # a negative flux flips both parts; 0 - F si with si = +0 and F < 0 is +0 - (-0) = +0
    negative = host.PredictHost()(freqs, delays, -np.ones((3, 1), f32))[0]
    assert negative[2].tolist() == [-1, 1, -1, 1, -1, 1, -1, 1]
    assert not np.signbit(negative[2].imag[[0, 2, 4, 6]]).any()


def test_delays():
    rs = np.random.RandomState(3)
    uvw = rs.uniform(-8000, 8000, (30, 3))
    lm = rs.uniform(-0.02, 0.02, (4, 2))
    lm[0] = 0  # the phase centre
    got = host.PredictHost.delays(uvw, lm)
    assert got.shape == (4, 30) and got.dtype == np.float64 and not got[0].any()
    for s in range(4):
        for j in range(30):
            l, m = lm[s]
            u, v, w = uvw[j]
            want = (u * l + v * m + w * (math.sqrt(1 - l * l - m * m) - 1)) / 299792458.0
            assert got[s, j] == pytest.approx(want, rel=1e-14, abs=1e-22)
    assert host.PredictHost.delays(uvw[:1], [[0.6, 0.0]])[0, 0] == pytest.approx(
        (uvw[0, 0] * 0.6 - uvw[0, 2] * 0.2) / 299792458.0, rel=1e-12)  # fmt: skip
    assert host.PredictHost.delays([[1.0, 2.0, 299792458.0]], [[0.0, 1.0]])[0, 0] == pytest.approx(
        2.0 / 299792458.0 - 1.0, rel=1e-14)  # fmt: skip
    assert host.PredictHost.delays(uvw.astype(np.float32), lm.tolist()).dtype == np.float64
    for bad_lm in ([[0.8, 0.7]], [[0.0, 0.0], [-1.0, 0.1]], [[np.nan, 0.0]]):
        with pytest.raises(ValueError, match="l\\^2 \\+ m\\^2 > 1"):
            host.PredictHost.delays(uvw, bad_lm)
    for bad_uvw in (uvw[:, :2], uvw[0], uvw.T):
        with pytest.raises(ValueError, match="uvw"):
            host.PredictHost.delays(bad_uvw, lm)
    for bad_lm in (lm[:, :1], lm[0], np.zeros((4, 3))):
        with pytest.raises(ValueError, match="lm"):
            host.PredictHost.delays(uvw, bad_lm)


# --------------------------------------------------------------------------------- division
def divide_one(freqs, delays, flux, flag_value=64):
    """One channel: every baseline with vis 1 + 2j, weight 4, flags 3."""
    delays = np.atleast_2d(np.asarray(delays, np.float64))
    baselines = delays.shape[1]
    vis = np.full((1, baselines), 1 + 2j, np.complex64)
    vis[0, 0] = complex(np.nan, -0.0)  # (kept bit for bit where there is no model)
    with np.errstate(all="ignore"):
        out = host.PredictHost(flag_value)(
            np.asarray(freqs, np.float64), delays, np.asarray(flux, f32).reshape(1, -1), vis,
            np.full((1, baselines), 4, f32), np.full((1, baselines), 3, np.uint8))  # fmt: skip
    return vis, out


@pytest.mark.parametrize("freqs, delays, flux", [
    ([1e9], [[1e-7, 2e-7, 0.0]], [0.0]),  # M = 0
    ([1e9], [[1e-7, 2e-7, 0.0]], [-0.0]),
    ([1e9], [[1e-7, 2e-7, 0.0]], [1e-30]),  # d underflows to 0
    ([1e9], [[1e-7, 2e-7, 0.125e-9]], [3e38]),  # d overflows (and so does re + im at 1/8 turn)
    ([np.nan], [[1e-7, 2e-7, 0.0]], [1.0]),
    ([np.inf], [[1e-7, 2e-7, 0.0]], [1.0]),
    ([1e9], [[np.nan, -np.inf, np.inf]], [1.0]),
    ([1e9], [[1e-7, 2e-7, 0.0]], [np.nan]),
    ([1e9], [[1e-7, 2e-7, 0.0]], [np.inf]),  # (inf * co with co = 0 exactly, or d = inf)
    ([1e9], [[1e-7, 2e-7, 0.0], [1e-7, 2e-7, 0.0]], [1.5, -1.5]),  # two sources that cancel
    ([1e9], [[1e-7, 2e-7, 0.0], [3e-7, 0.0, 5e-7], [1e-7, 2e-7, 0.0]], [2.5, 0.0, -2.5]),
])  # fmt: skip
def test_no_usable_model(freqs, delays, flux):
    vis, (model, out_vis, out_weights, out_flags) = divide_one(freqs, delays, flux)
    with np.errstate(all="ignore"):
        d = model.real * model.real + model.imag * model.imag
    assert not ((d > 0) & (d < np.inf)).any()
    assert_same(vis, out_vis, "vis is kept bit for bit")
    assert not out_weights.any() and not np.signbit(out_weights).any()
    assert (out_flags == (3 | 64)).all()


def test_division_where_ok():
    """Weight and flags pass through: w d and the flags as they were; vis / M."""
    delays = [[0.0, 0.25, 0.5, 0.125], [0.0, 0.0, 0.0, 0.0]]
    vis, (model, out_vis, out_weights, out_flags) = divide_one([1.0], delays, [2.0, 1.0])
    assert model.tolist() == [[3, 1 - 2j, -1, complex(f32(1 + 2 * SQRT_HALF), -f32(2 * SQRT_HALF))]]
    # (1 + 2j) / (1 - 2j) = (-3 + 4j) / 5, (1 + 2j) / -1
    assert out_vis[0, 1] == complex(f32(-3) / f32(5), f32(4) / f32(5)) and out_vis[0, 2] == -1 - 2j
    assert np.isnan(out_vis[0, 0].real) and out_vis[0, 0].imag != out_vis[0, 0].imag  # NaN / 9
    assert out_weights.tolist()[0][:3] == [36, 20, 4] and (out_flags == 3).all()
    d3 = f32(model[0, 3].real * model[0, 3].real) + f32(model[0, 3].imag * model[0, 3].imag)
    assert out_weights[0, 3] == f32(4) * d3
    # one sample without a model among them changes nothing for the others
    vis2, out2 = divide_one([1.0], delays, [2.0, 2.0], 128)
    assert out2[0][0, 2] == 0 and out2[1][0, 2] == 1 + 2j
    assert out2[2][0].tolist()[2] == 0 and out2[3].tolist() == [[3, 3, 131, 3]]


# --------------------------------------------------------------------------------- recovery
#: the largest relative difference from the true gains measured in test_recovers_the_gains
#:
MEASURED_RECOVERY = 2.06e-6


def recovery_case():
    """12 inputs, 3 sources up to 0.01 rad off centre, 5 channels: noise-free data from float64
    gains and the longdouble model."""
    n_inputs, channels = 12, 5
    rs = np.random.RandomState(12)
    antennas = rs.uniform(-500, 500, (n_inputs, 3)) * [1, 1, 0.02]
    inputs = np.array(np.triu_indices(n_inputs, 1)).T.astype(np.int32)
    uvw = antennas[inputs[:, 0]] - antennas[inputs[:, 1]]
    lm = np.array([[0.0, 0.0], [0.006, -0.004], [-0.003, 0.008]])
    delays = host.PredictHost.delays(uvw, lm)
    freqs = np.linspace(1.2e9, 1.6e9, channels)
    flux = (np.array([[5.0, 1.5, 0.7]]) * (freqs[:, np.newaxis] / 1.4e9) ** [[-0.7, -0.3, -1.1]])
    flux = flux.astype(f32)
    truth = gen_solve.make_gains(7, channels, n_inputs, span=1.0).astype(np.complex128)
    reference = gen.reference_model(freqs, delays, flux).astype(np.complex128)
    vis = (truth[:, inputs[:, 0]] * np.conj(truth[:, inputs[:, 1]]) * reference)
    return freqs, delays, flux, vis.astype(np.complex64), inputs, truth


def test_recovers_the_gains():
    """PredictHost (divide) -> SolveGainsHost(200, 1e-6) recovers the gains of noise-free data
    from an off-centre, three-source field; the same solve on the undivided data does not."""
    freqs, delays, flux, vis, inputs, truth = recovery_case()
    n_inputs = truth.shape[1]
    pairs = host.SolveGainsHost.pair_table(inputs, n_inputs)
    weights = np.ones(vis.shape, f32)
    flags = np.zeros(vis.shape, np.uint8)
    _, out_vis, out_weights, out_flags = host.PredictHost()(freqs, delays, flux, vis, weights, flags)
    assert not out_flags.any() and (out_weights > 0).all()
    solve = host.SolveGainsHost(200, 1e-6)
    turned = truth * np.conj(truth[:, :1]) / np.abs(truth[:, :1])

    def worst(gains):
        return float(np.abs(gains - turned).max() / np.abs(turned).max())

    gains, iterations, status = solve(out_vis, pairs, out_weights, out_flags)
    assert not status.any()
    divided, undivided = worst(gains), worst(solve(vis, pairs, weights, flags)[0])
    print(f"largest relative difference from the true gains: {divided:.3e} with the model, "
          f"{undivided:.3e} without")  # fmt: skip
    assert divided <= 2 * MEASURED_RECOVERY
    assert undivided > 0.1


# ----------------------------------------------------------------------------------- errors
def test_host_errors():
    for bad in (0, 256, -1):
        with pytest.raises(ValueError, match="flag_value"):
            host.PredictHost(bad)
    for bad in (1.0, True, "1"):
        with pytest.raises(TypeError, match="flag_value"):
            host.PredictHost(bad)
    assert host.PredictHost().flag_value == 64 and host.PredictHost(255).flag_value == 255
    assert host.PredictHost.MAX_SOURCES == 64
    fn = host.PredictHost()
    good = gen.make_case(1, 4, 6, 3)
    fn(**good)
    bads = {
        "freqs": [good["freqs"].astype(f32), good["freqs"].reshape(4, 1), np.zeros(0)],
        "delays": [good["delays"].astype(f32), good["delays"][0], np.zeros((0, 6)),
                   np.zeros((65, 6)), np.zeros((3, 0))],
        "flux": [good["flux"].astype(np.float64), good["flux"][:3], good["flux"][:, :2],
                 good["flux"].T, good["flux"][0]],
        "vis": [good["vis"].astype(np.complex128), good["vis"][0], good["vis"][:, :5],
                good["vis"].T],
        "weights": [good["weights"].astype(np.float64), good["weights"][:, :5], good["weights"][0]],
        "flags": [good["flags"].astype(np.int8), good["flags"][:3], good["flags"][0]],
    }  # fmt: skip
    for name, values in bads.items():
        for bad in values:
            with pytest.raises(ValueError, match=name):
                fn(**{**good, name: bad})
    for name in ("weights", "flags"):
        with pytest.raises(ValueError, match=f"{name} given without vis"):
            fn(good["freqs"], good["delays"], good["flux"], **{name: good[name]})
    fn(good["freqs"], np.zeros((64, 6)), np.zeros((4, 64), f32))


def test_template_and_operation_errors(context, queue):
    with pytest.raises(ValueError):
        ingest.PredictTemplate(context, tuning={"wgs": 256})
    assert ingest.PredictTemplate(context, tuning={}).tuning == {}
    assert ingest.PredictTemplate.autotune(context) == {}
    assert ingest.PredictTemplate.TUNING_KEYS == ()
    assert ingest.PredictTemplate.host_class is host.PredictHost
    assert ingest.PredictTemplate.KERNEL == "ksp_predict"
    assert ingest.PredictTemplate.operation_class is ingest.Predict
    with pytest.raises(ValueError, match="model and divide"):
        ingest.PredictTemplate(context, model=False, divide=False)
    for bad in (0, 256, -128):
        with pytest.raises(ValueError, match="flag_value"):
            ingest.PredictTemplate(context, flag_value=bad)
    with pytest.raises(TypeError, match="flag_value"):
        ingest.PredictTemplate(context, flag_value=1.5)
    template = ingest.PredictTemplate(context)
    assert template.kernel.name == "ksp_predict"
    assert (template.model, template.divide, template.weights, template.flags,
            template.flag_value) == (True, False, False, False, 64)  # fmt: skip
    template = ingest.PredictTemplate(context, divide=True)
    assert (template.weights, template.flags) == (True, True)
    for args in [(0, 4, 2), (4, 0, 2), (-4, 4, 2), (4, -1, 2), (4, 4, 0), (4, 4, -1), (4, 4, 65)]:
        with pytest.raises(ValueError):
            template.instantiate(queue, *args)
    assert isinstance(template.instantiate(queue, 4, 5, 64), ingest.Predict)
    fn = template.instantiate(queue, 1, 1, 1)
    assert fn.parameters() == {"model": True, "divide": True, "weights": True, "flags": True,
                               "flag_value": 64, "n_sources": 1, "channels": 1, "baselines": 1}  # fmt: skip


def test_host_from_device(context, queue):
    case = gen.make_case(1, 4, 5, 3)
    model_args = (case["freqs"], case["delays"], case["flux"])
    for model, divide, weights, flags in VARIANTS:
        template = ingest.PredictTemplate(context, model, divide, weights, flags)
        adapter = ingest.PredictHostFromDevice(template, queue)
        given = {"vis": case["vis"] if divide else None,
                 "weights": case["weights"] if weights else None,
                 "flags": case["flags"] if flags else None}  # fmt: skip
        del queue.launches[:]
        out = adapter(*model_args, **given)
        assert len(out) == 4
        assert [o is not None for o in out] == [model, divide, weights, flags]
        for o, dtype in zip(out, (np.complex64, np.complex64, f32, np.uint8)):
            assert o is None or (o.shape, o.dtype) == ((4, 5), dtype)
        assert [name for name, _ in queue.launches] == ["ksp_predict"]
        assert [int(a) for a in queue.launches[0][1][10:13]] == [4, 5, 3]
        # each optional input exactly when the template has it
        for name in given:
            wrong = dict(given)
            wrong[name] = None if given[name] is not None else case[name]
            with pytest.raises(TypeError, match=name):
                adapter(*model_args, **wrong)
    adapter = ingest.PredictHostFromDevice(ingest.PredictTemplate(context), queue)
    with pytest.raises(ValueError):
        adapter(case["freqs"], np.zeros((65, 5)), np.zeros((4, 65), f32))
    with pytest.raises(ValueError):
        adapter(np.zeros(0), case["delays"], case["flux"][:0])


# ----------------------------------------------------------------------------------- wiring
def expected_slots(model, divide, weights, flags):
    names = ["freqs", "delays", "flux"] + (["model"] if model else [])
    names += ["vis", "out_vis"] if divide else []
    names += ["weights", "out_weights"] if weights else []
    names += ["flags", "out_flags"] if flags else []
    return names


DTYPES = {"model": np.complex64, "vis": np.complex64, "weights": np.float32, "flags": np.uint8}


@pytest.mark.parametrize("model, divide, weights, flags", VARIANTS)
def test_slots(model, divide, weights, flags, context, queue):
    template = ingest.PredictTemplate(context, model, divide, weights, flags, flag_value=4)
    fn = template.instantiate(queue, 300, 200, 58)
    assert list(fn.slots) == expected_slots(model, divide, weights, flags)
    for name, slot in fn.slots.items():
        if name == "freqs":
            assert (slot.shape, slot.dtype) == ((300,), np.float64)
        elif name == "delays":
            assert (slot.shape, slot.dtype) == ((58, 200), np.float64)
        elif name == "flux":
            assert (slot.shape, slot.dtype) == ((300, 58), np.float32)
        else:
            assert (slot.shape, slot.dtype) == ((300, 200), DTYPES[name.replace("out_", "")])
    # a dimension object of its own for everything that can be padded
    dims = [d for slot in fn.slots.values() for d in slot.dimensions]
    assert len({id(d) for d in dims}) == len(dims) == 2 * len(fn.slots) - 1
    assert fn.parameters() == {"model": model, "divide": divide, "weights": weights,
                               "flags": flags, "flag_value": 4, "n_sources": 58,
                               "channels": 300, "baselines": 200}  # fmt: skip
    # weights and flags only matter with divide
    ignored = ingest.PredictTemplate(context, True, False, True, True).instantiate(queue, 3, 4, 5)
    assert list(ignored.slots) == ["freqs", "delays", "flux", "model"]


@pytest.mark.parametrize("model, divide, weights, flags, in_place", [
    variant + (in_place,) for variant in VARIANTS for in_place in (False, True)
    if variant[1] or not in_place])  # fmt: skip
def test_launch_arguments(model, divide, weights, flags, in_place, context, queue):
    template = ingest.PredictTemplate(context, model, divide, weights, flags, flag_value=32)
    fn = template.instantiate(queue, 300, 200, 58)
    kinds = (["vis"] if divide else []) + (["weights"] if weights else []) + (
        ["flags"] if flags else [])  # fmt: skip
    if in_place:
        for kind in kinds:
            accel.Dimension(200, min_padded_size=500).link(fn.slots[kind].dimensions[1])
            fn.slots[kind].dimensions[1].link(fn.slots["out_" + kind].dimensions[1])
        fn.ensure_all_bound()
        fn.bind(**{"out_" + kind: fn.buffer(kind) for kind in kinds})
    else:
        accel.Dimension(200, min_padded_size=500).link(fn.slots["delays"].dimensions[1])
    fn()
    assert [name for name, _ in queue.launches] == ["ksp_predict"]
    args = queue.launches[0][1]
    assert len(args) == 23
    present = {"model": model, "vis": divide, "weights": weights, "flags": flags,
               "out_vis": divide, "out_weights": weights, "out_flags": flags}  # fmt: skip

    def buf(name):
        return fn.buffer(name).buffer if present.get(name, True) else None

    order = ["freqs", "delays", "flux", "model", "vis", "weights", "flags", "out_vis",
             "out_weights", "out_flags"]  # fmt: skip
    for got, name in zip(args[:10], order):
        assert got is buf(name), name
    for kind in kinds:
        assert (fn.buffer(kind) is fn.buffer("out_" + kind)) == in_place
    assert all(isinstance(a, np.int32) for a in args[10:])
    assert [int(a) for a in args[10:13]] == [300, 200, 58]

    def stride(name):
        return fn.buffer(name).padded_shape[1] if present.get(name, True) else 0

    strides = [stride(name) for name in order[1:]]
    assert [int(a) for a in args[13:22]] == strides
    pad = {"vis": 208, "weights": 224, "flags": 256}  # whole 128-byte rows
    if in_place:
        want = [512 if present[kind] else 0 for kind in ("vis", "weights", "flags")]
        assert strides == [208, 64, 208 if model else 0] + want + want
    else:
        want = [pad[kind] if present[kind] else 0 for kind in ("vis", "weights", "flags")]
        assert strides == [512, 64, 208 if model else 0] + want + want
    assert int(args[22]) == 32


def test_in_place_binding(context, queue):
    """One buffer bound to vis and out_vis: both launch arguments are that buffer."""
    fn = ingest.PredictTemplate(context, False, True, False, False).instantiate(queue, 8, 40, 2)
    fn.slots["vis"].dimensions[1].link(fn.slots["out_vis"].dimensions[1])
    fn.ensure_all_bound()
    fn.bind(out_vis=fn.buffer("vis"))
    fn()
    args = queue.launches[0][1]
    assert args[4] is args[7] is fn.buffer("vis").buffer and args[3] is None
    assert int(args[16]) == int(args[19]) == fn.buffer("vis").padded_shape[1]


def test_between_finalise_and_solve(context, queue):
    """finalise -> predict -> solve -> apply_gains: predict divides what finalise left, solve
    reads predict's outputs, and apply_gains reads finalise's: it applies the gains to the
    data, not to the data divided by the model."""
    channels, baselines, cf, n_inputs, n_sources = 256, 66, 4, 12, 3
    rows = channels // cf
    finalise = device.FinaliseTemplate(context, channel_factor=cf).instantiate(
        queue, channels, baselines)  # fmt: skip
    predict = ingest.PredictTemplate(context, model=False, divide=True).instantiate(
        queue, rows, baselines, n_sources)  # fmt: skip
    solve = ingest.SolveGainsTemplate(context, corrections=True).instantiate(
        queue, rows, baselines, n_inputs)  # fmt: skip
    apply_gains = ingest.ApplyGainsTemplate(context).instantiate(queue, rows, baselines, n_inputs)
    accel.Dimension(baselines, min_padded_size=300).link(finalise.slots["weights"].dimensions[1])
    accel.Dimension(baselines, min_padded_size=700).link(solve.slots["weights"].dimensions[1])
    seq = accel.OperationSequence(
        queue, [("finalise", finalise), ("predict", predict), ("solve", solve),
                ("apply_gains", apply_gains)],
        compounds={"vis": ["finalise:vis", "predict:vis", "apply_gains:vis"],
                   "weights": ["finalise:weights", "predict:weights", "apply_gains:weights"],
                   "flags": ["finalise:flags", "predict:flags", "apply_gains:flags"],
                   "unit_vis": ["predict:out_vis", "solve:vis"],
                   "unit_weights": ["predict:out_weights", "solve:weights"],
                   "unit_flags": ["predict:out_flags", "solve:flags"],
                   "gains": ["solve:gains", "apply_gains:gains"]})  # fmt: skip
    assert {"vis", "weights", "flags", "unit_vis", "unit_weights", "unit_flags", "gains",
            "predict:freqs", "predict:delays", "predict:flux", "solve:pairs",
            "apply_gains:inputs", "apply_gains:out_vis"} <= set(seq.slots)  # fmt: skip
    assert "predict:model" not in seq.slots
    seq()
    assert [name for name, _ in queue.launches] == [
        "ksp_average_finalise", "ksp_predict", "ksp_solve_gains", "ksp_apply_gains"]  # fmt: skip
    final_args, predict_args, solve_args, gains_args = (launch[1] for launch in queue.launches)
    for i, name in enumerate(("vis", "weights", "flags")):
        averaged = seq.buffer(name).buffer
        assert final_args[3 + i] is predict_args[4 + i] is gains_args[i] is averaged
        unit = seq.buffer("unit_" + name).buffer
        assert predict_args[7 + i] is solve_args[i] is unit and unit is not averaged
    assert predict_args[3] is None
    assert solve_args[5] is gains_args[3] is seq.buffer("gains").buffer
    assert int(final_args[14]) == int(predict_args[17]) == int(gains_args[12]) == 320
    assert int(predict_args[20]) == int(solve_args[12]) == 704
    assert int(predict_args[16]) == int(gains_args[11]) == seq.buffer("vis").padded_shape[1]
    assert int(predict_args[19]) == int(solve_args[11]) == seq.buffer("unit_vis").padded_shape[1]
    assert [int(a) for a in predict_args[10:13]] == [rows, baselines, n_sources]


# ------------------------------------------------------------------- the launcher's checks
@pytest.fixture(scope="module")
def lib():
    from katsdpsigproc_amd import _lib, build_native

    if not os.path.exists(_lib.LIB_PATH):
        build_native.build()
    return _lib.load()


POINTERS = ["freqs", "delays", "flux", "model", "vis", "weights", "flags", "out_vis",
            "out_weights", "out_flags"]  # fmt: skip
STRIDES = ["delays", "flux", "model", "vis", "weights", "flags", "out_vis", "out_weights",
           "out_flags"]  # fmt: skip


def test_argument_validation_without_gpu(lib):
    from katsdpsigproc_amd import _lib

    # never dereferenced: every call below fails its checks first. Ten arrays far apart.
    p = {name: ctypes.c_void_p((i + 1) << 32) for i, name in enumerate(POINTERS)}

    def call(channels=4, baselines=8, n_sources=3, flag_value=64, device=0, **changed):
        a = dict(p, **{name + "_stride": 8 for name in STRIDES})
        a["flux_stride"] = 3
        a.update(changed)
        rc = lib.ksp_predict(device, None, *(a[name] for name in POINTERS), channels, baselines,
                             n_sources, *(a[name + "_stride"] for name in STRIDES), flag_value)  # fmt: skip
        assert rc != 0
        return _lib.last_error()

    none_w = dict(weights=None, out_weights=None, weights_stride=0, out_weights_stride=0)
    none_f = dict(flags=None, out_flags=None, flags_stride=0, out_flags_stride=0)
    none_v = dict(vis=None, out_vis=None, vis_stride=0, out_vis_stride=0)
    for name in ("freqs", "delays", "flux"):
        assert f"invalid argument: {name} is NULL" in call(**{name: None})
    assert "invalid argument: model and vis must not both be NULL" in call(
        model=None, **none_v, **none_w, **none_f)  # fmt: skip
    for name in ("vis", "out_vis"):
        assert "vis and out_vis must both be NULL or both be given" in call(
            **{name: None}, **none_w, **none_f)  # fmt: skip
    for name in ("weights", "out_weights"):
        assert "weights and out_weights must both be NULL or both be given" in call(**{name: None})
    for name in ("flags", "out_flags"):
        assert "flags and out_flags must both be NULL or both be given" in call(**{name: None})
    assert "invalid argument: weights needs vis" in call(**none_v)
    assert "invalid argument: flags needs vis" in call(**none_v, **none_w)
    for bad in (0, -1):
        assert "invalid argument: channels must be at least 1" in call(channels=bad)
        assert "invalid argument: baselines must be at least 1" in call(baselines=bad)
    for bad in (0, -1, 65):
        assert "invalid argument: n_sources must be 1..64" in call(n_sources=bad, flux_stride=65)
    for bad in (0, 256, -128):
        assert "invalid argument: flag_value must be 1..255" in call(flag_value=bad)
    for name in STRIDES:
        what = "n_sources" if name == "flux" else "baselines"
        assert f"invalid argument: {name}_stride is smaller than {what}" in call(
            **{name + "_stride": 2})
    assert "flux_stride is smaller" in call(n_sources=64, flux_stride=63)
    # the order of the checks: everything wrong at once, then only the numbers and strides
    strides = {name + "_stride": -1 for name in STRIDES}
    assert "invalid argument: freqs is NULL" in call(
        channels=0, baselines=0, n_sources=0, flag_value=0, **dict.fromkeys(p), **strides)
    assert "invalid argument: channels must be at least 1" in call(
        channels=0, baselines=0, n_sources=0, flag_value=0, **strides)
    assert "invalid argument: delays_stride is smaller than baselines" in call(**strides)
    assert "invalid argument: flux_stride is smaller than n_sources" in call(
        **dict(strides, delays_stride=8))  # fmt: skip
    assert "invalid argument: model_stride is smaller than baselines" in call(
        **dict(strides, delays_stride=8, flux_stride=3))  # fmt: skip
    # an absent array's stride is not looked at: the call gets as far as the next check
    assert "vis_stride is smaller" in call(**none_w, **none_f, model=None, model_stride=-1,
                                           vis_stride=7)  # fmt: skip
    assert "n_sources" in call(**none_v, **none_w, **none_f, n_sources=0)

    # an output that overlaps its input without being it
    def at(name, offset):
        return ctypes.c_void_p(p[name].value + offset)

    item = {"vis": 8, "weights": 4, "flags": 1}
    for kind, size in item.items():
        message = f"out_{kind} overlaps {kind} without being {kind} with the same stride"
        extent = (3 * 8 + 8) * size  # the bytes from the first element to the last
        out = "out_" + kind
        assert message in call(**{out: at(kind, size)})
        assert message in call(**{out: at(kind, extent - 1)})
        assert message in call(**{out: at(kind, -(extent - 1))})
        assert message in call(**{out: p[kind], out + "_stride": 9})  # same pointer, other stride
    # model shares no byte with anything, not even as the same array
    extents = {"freqs": 4 * 8, "delays": (2 * 8 + 8) * 8, "flux": (3 * 3 + 3) * 4}
    extents.update({name: (3 * 8 + 8) * {"w": 4, "f": 1}.get(name.replace("out_", "")[0], 8)
                    for name in POINTERS[4:]})  # fmt: skip
    model_extent = (3 * 8 + 8) * 8
    for name, extent in extents.items():
        message = f"invalid argument: model overlaps {name}"
        assert message in call(model=p[name])
        assert message in call(model=at(name, extent - 1))
        assert message in call(model=at(name, -(model_extent - 1)))
    # in place, and arrays that only touch, pass every check: what is left to fail is the
    # first device call, which device -1 fails on any machine
    for touching in (dict(out_vis=p["vis"], out_weights=p["weights"], out_flags=p["flags"]),
                     dict(model=at("vis", model_extent), out_vis=at("vis", -model_extent)),
                     dict(model=at("freqs", 4 * 8)), dict(model=at("flux", -model_extent))):  # fmt: skip
        assert "hipSetDevice(device) failed" in call(device=-1, **touching)
    assert "hipSetDevice(device) failed" in call(device=-1, model=None, **none_w, **none_f)
    assert "hipSetDevice(device) failed" in call(device=-1, **none_v, **none_w, **none_f)


def test_header_binding_and_exports_agree(lib):
    from katsdpsigproc_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "katsdpsigproc_hip.h")).read()
    comment = re.search(r"/\* predict:.*?\*/", text, re.S).group(0)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declaration = re.search(r"int ksp_predict\((.*?)\);", text, re.S)
    assert declaration is not None
    parameters = [" ".join(part.split()) for part in declaration.group(1).split(",")]
    argtypes = _lib.SIGNATURES["ksp_predict"]
    assert len(parameters) == len(argtypes) == 25
    for parameter, argtype in zip(parameters, argtypes):
        assert ("*" in parameter) == (argtype is ctypes.c_void_p), parameter
        assert argtype in (ctypes.c_int, ctypes.c_void_p)
    names = [parameter.replace("*", " ").split()[-1] for parameter in parameters]
    assert names == ["device", "stream"] + POINTERS + ["channels", "baselines", "n_sources"] + [
        name + "_stride" for name in STRIDES] + ["flag_value"]  # fmt: skip
    assert hasattr(lib, "ksp_predict") and "ksp_predict" in _lib.declared_symbols()
    assert lib.ksp_abi_version() == _lib.ABI_VERSION == 5
    for name in ("PredictTemplate", "Predict", "PredictHostFromDevice"):
        assert hasattr(ingest, name)
    assert hasattr(host, "PredictHost")
    # the header comment, the host class and the one copy of the series (in its comment and in
    # its code) show the same digits; the kernel includes that copy and has none of its own
    csrc = os.path.join(root, "katsdpsigproc_amd", "csrc")
    series = open(os.path.join(csrc, "cal_math.h")).read()
    kernel = open(os.path.join(csrc, "predict.hip")).read()
    assert '#include "cal_math.h"' in kernel and "ksp_cos_sin_turns(" in kernel
    coefficients = host.PredictHost.SIN_COEFFICIENTS + host.PredictHost.COS_COEFFICIENTS
    for value in coefficients + (host.PredictHost.TWO_PI,):
        assert repr(abs(value)) in comment and series.count(repr(abs(value))) >= 2, value
    for value in coefficients + (host.PredictHost.TWO_PI,):
        if abs(value) not in (1.0, 0.5):  # (digits that text has for other reasons)
            assert repr(abs(value)) not in kernel, value
    for k in range(6):
        assert host.PredictHost.SIN_COEFFICIENTS[k] == (-1) ** k / math.factorial(2 * k + 1)
    for k in range(7):
        assert host.PredictHost.COS_COEFFICIENTS[k] == (-1) ** k / math.factorial(2 * k)
