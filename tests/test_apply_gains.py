"""Applying gains without a GPU: ``rfi.host.ApplyGainsHost`` against a triple loop of float32
scalars and known answers, argument errors, slot lists and every launch argument of every variant
on the fake backend, the sequence finalise -> apply_gains -> compress, and the argument checks
of ``ksp_apply_gains``, which come before any device call."""

import ctypes
import os
import re

import numpy as np
import pytest

from katsdpsigproc_amd import accel
from katsdpsigproc_amd.rfi import device, host, ingest
from tests import inputs_apply_gains as gen
from tests.fakes import FakeContext
from tests.inputs_apply_gains import assert_same

f32 = np.float32
VARIANTS = [(True, True), (True, False), (False, True), (False, False)]


@pytest.fixture
def context():
    return FakeContext()


@pytest.fixture
def queue(context):
    return context.create_command_queue()


# --------------------------------------------------------------------------- the triple loop
def triple_loop(vis, gains, inputs, weights, flags, flag_value):
    """The definition, sample by sample and step by step, in np.float32 scalars."""
    channels, baselines = vis.shape
    n_inputs = gains.shape[1]
    out_vis = np.empty_like(vis)
    out_weights = np.empty_like(weights)
    out_flags = np.empty_like(flags)
    nan = np.isnan
    with np.errstate(all="ignore"):
        for c in range(channels):
            for j in range(baselines):
                a, b = int(inputs[j, 0]), int(inputs[j, 1])
                inr = 0 <= a < n_inputs and 0 <= b < n_inputs
                ok = False
                if inr:
                    ga, gb = gains[c, a], gains[c, b]
                    gar, gai, gbr, gbi = f32(ga.real), f32(ga.imag), f32(gb.real), f32(gb.imag)
                    cr = f32(f32(gar * gbr) + f32(gai * gbi))
                    ci = f32(f32(gai * gbr) - f32(gar * gbi))
                    ok = not nan(cr) and not nan(ci)
                if ok:
                    p = f32(f32(cr * cr) + f32(ci * ci))
                    re, im = f32(vis[c, j].real), f32(vis[c, j].imag)
                    out_vis[c, j] = complex(f32(f32(re * cr) - f32(im * ci)),
                                            f32(f32(re * ci) + f32(im * cr)))  # fmt: skip
                    out_weights[c, j] = f32(weights[c, j] / p) if p > 0 else f32(0)
                    out_flags[c, j] = flags[c, j]
                else:
                    out_vis[c, j] = vis[c, j]
                    out_weights[c, j] = 0
                    out_flags[c, j] = flags[c, j] | flag_value
    return out_vis, out_weights, out_flags


@pytest.mark.parametrize("channels, baselines, n_inputs, pattern, flag_value", [
    (9, 41, 7, "outside", 128), (5, 33, 64, "random", 1), (4, 20, 3, "auto", 255),
    (1, 1, 1, "one", 16), (3, 40, 70, "stride32", 128)])  # fmt: skip
def test_host_against_triple_loop(channels, baselines, n_inputs, pattern, flag_value):
    case = gen.make_case(channels * 100 + baselines, channels, baselines, n_inputs, pattern,
                         flag_value)  # fmt: skip
    before = {name: value.copy() for name, value in case.items()}
    fn = host.ApplyGainsHost(flag_value)
    got = fn(case["vis"], case["gains"], case["inputs"], case["weights"], case["flags"])
    want = triple_loop(flag_value=flag_value, **case)
    for name, w, g in zip(("out_vis", "out_weights", "out_flags"), want, got):
        assert_same(w, g, name)
        assert g.flags.c_contiguous
    for name, value in case.items():  # the inputs are never modified
        assert_same(before[name], value, name)
    # each optional array on its own gives the same answers
    only_w = fn(case["vis"], case["gains"], case["inputs"], weights=case["weights"])
    only_f = fn(case["vis"], case["gains"], case["inputs"], flags=case["flags"])
    neither = fn(case["vis"], case["gains"], case["inputs"])
    assert only_w[2] is None and only_f[1] is None and neither[1] is None and neither[2] is None
    for other in (only_w, only_f, neither):
        assert_same(got[0], other[0], "out_vis")
    assert_same(got[1], only_w[1], "out_weights")
    assert_same(got[2], only_f[2], "out_flags")


def test_generators_cover_the_cases():
    gains = gen.make_gains(3, 64, 128)
    re, im = gains.real, gains.imag
    assert (np.isnan(re) & ~np.isnan(im)).any() and (~np.isnan(re) & np.isnan(im)).any()
    assert np.isposinf(re).any() and np.isneginf(im).any()
    assert ((re == 0) & (im == 0)).any()
    tiny = np.finfo(f32).tiny
    assert ((np.abs(re) > 0) & (np.abs(re) < tiny)).any()
    assert (re == f32(1e-30)).any() and (re == f32(1e30)).any()
    ordinary = np.abs(gen.make_gains(3, 64, 128, special=False))
    assert ordinary.min() < 2.0**-18 and ordinary.max() > 2.0**18
    with np.errstate(all="ignore"):
        assert f32(1e-30) * f32(1e-30) == 0 and np.isinf(f32(1e30) * f32(1e30))
    outside = gen.make_inputs(5, "outside", 400, 9)
    for bad in (-1, 9, gen.INT32_MIN, gen.INT32_MAX):
        assert (outside[:, 0] == bad).any() and (outside[:, 1] == bad).any()
    assert ((outside >= 0) & (outside < 9)).all(axis=1).sum() > 200
    one = gen.make_inputs(5, "one", 40, 9)
    assert len(np.unique(one)) == 1
    auto = gen.make_inputs(5, "auto", 40, 9)
    assert (auto[:, 0] == auto[:, 1]).all() and len(np.unique(auto)) > 3
    stride = gen.make_inputs(5, "stride32", 40, 4096)
    assert (np.diff(stride[:, 0]) % 4096 == 32).all()
    for pattern in gen.PATTERNS:
        made = gen.make_inputs(1, pattern, 17, 5)
        assert made.dtype == np.int32 and made.shape == (17, 2) and made.flags.c_contiguous
    vis = gen.make_vis(2, 50, 60)
    assert np.isnan(vis.real).any() and np.isinf(vis.imag).any()
    assert ((vis.real == 0) & np.signbit(vis.real)).any() and ((vis.real == 0) & ~np.signbit(vis.real)).any()
    weights = gen.make_weights(2, 50, 60)
    assert (weights == 0).any() and (weights == 2.0**30).any() and (weights == f32(2.0**-30)).any()
    flags = gen.make_flags(2, 50, 60, 4)
    assert (flags & 4).any() and (flags == 0).any() and len(np.unique(flags)) > 100


# ------------------------------------------------------------------------- known answers
def c64(rows):
    return np.array(rows, np.complex64)


def test_unit_gains_leave_finite_data_unchanged():
    vis = gen.make_vis(7, 6, 50)
    finite = np.isfinite(vis.real) & np.isfinite(vis.imag)
    vis[~finite] = complex(-0.0, 2.0**-140)
    weights = gen.make_weights(8, 6, 50)
    flags = gen.make_flags(9, 6, 50)
    gains = np.ones((6, 5), np.complex64)
    inputs = gen.make_inputs(1, "random", 50, 5)
    out = host.ApplyGainsHost()(vis, gains, inputs, weights, flags)
    # v * 1 - v' * 0 keeps every finite value, denormals included, but for the sign of a zero
    assert_same(np.where(vis.real == 0, f32(0), vis.real), np.where(out[0].real == 0, f32(0), out[0].real))
    assert_same(np.where(vis.imag == 0, f32(0), vis.imag), np.where(out[0].imag == 0, f32(0), out[0].imag))
    nonzero = (vis.real != 0) & (vis.imag != 0)
    assert nonzero.sum() > 200
    assert_same(vis[nonzero], out[0][nonzero], "vis")
    assert_same(weights, out[1], "weights")
    assert_same(flags, out[2], "flags")


def test_autocorrelation_ci_is_plus_zero():
    """ga conj(ga) has ci = ga.im ga.re - ga.re ga.im = +0 exactly, so a real visibility stays
    real (+0 imaginary part) and is scaled by |ga|^2 as float32 computes it."""
    gains = gen.make_gains(4, 5, 9, special=False)
    inputs = gen.make_inputs(4, "auto", 30, 9)
    vis = np.zeros((5, 30), np.complex64)
    vis.real[...] = 3.0
    out_vis, out_weights, _ = host.ApplyGainsHost()(vis, gains, inputs, np.ones((5, 30), f32))
    ga = gains[:, inputs[:, 0]]
    cr = ga.real * ga.real + ga.imag * ga.imag
    assert_same(f32(3.0) * cr, np.ascontiguousarray(out_vis.real), "re")
    assert not out_vis.imag.any() and not np.signbit(out_vis.imag).any()
    assert_same(f32(1) / (cr * cr + f32(0)), out_weights, "weights")


@pytest.mark.parametrize("gain", [complex(np.nan, 1), complex(1, np.nan), complex(np.inf, np.inf)])
def test_nan_gain_passes_vis_through(gain):
    """(inf + inf j) conj(itself): ci = inf - inf, a NaN correction like the others."""
    gains = c64([[2, gain, 1j]])
    inputs = np.array([[0, 1], [1, 2], [1, 1], [0, 2]], np.int32)
    vis = c64([[complex(np.nan, -0.0), complex(1.5, np.inf), 2 - 3j, 1 + 1j]])
    weights = np.array([[4, 5, 6, 8]], f32)
    flags = np.array([[1, 128, 0, 2]], np.uint8)
    out_vis, out_weights, out_flags = host.ApplyGainsHost(128)(vis, gains, inputs, weights, flags)
    assert_same(vis[:, :3], out_vis[:, :3], "vis passes through bit for bit")
    assert out_vis[0, 3] == (1 + 1j) * (2 * -1j)
    assert out_weights.tolist() == [[0, 0, 0, 2]]
    assert out_flags.tolist() == [[129, 128, 128, 2]]


def test_out_of_range_indices_behave_like_a_nan_gain():
    gains = c64([[2, 4], [1, 3]])
    bad = [-1, 2, gen.INT32_MIN, gen.INT32_MAX]
    inputs = np.array([[b, 0] for b in bad] + [[1, b] for b in bad] + [[b, b] for b in bad]
                      + [[1, 0]], np.int32)  # fmt: skip
    n = len(inputs)
    vis = gen.make_vis(1, 2, n)
    weights = np.full((2, n), 8, f32)
    flags = np.full((2, n), 3, np.uint8)
    out_vis, out_weights, out_flags = host.ApplyGainsHost(64)(vis, gains, inputs, weights, flags)
    assert_same(vis[:, :-1], out_vis[:, :-1], "vis passes through bit for bit")
    assert not out_weights[:, :-1].any() and (out_flags[:, :-1] == 67).all()
    assert out_weights[:, -1].tolist() == [f32(8) / f32(64), f32(8) / f32(9)]
    assert out_flags[:, -1].tolist() == [3, 3]


def test_zero_infinite_and_tiny_corrections():
    """A zero correction and one whose p underflows: weight 0 and no flag; an infinite p: a
    finite weight becomes 0, again no flag."""
    gains = c64([[0, 1, 1e-30, 1e30]])
    inputs = np.array([[0, 1], [2, 2], [3, 3], [3, 1]], np.int32)
    vis = c64([[1 + 2j, 1 + 2j, 1 + 2j, 1 + 0j]])
    weights = np.full((1, 4), 2, f32)
    flags = np.zeros((1, 4), np.uint8)
    with np.errstate(all="ignore"):
        out_vis, out_weights, out_flags = host.ApplyGainsHost()(vis, gains, inputs, weights, flags)
    assert not out_weights.any() and not out_flags.any()
    assert out_vis[0, 0] == 0 and np.isinf(out_vis[0, 2].real)
    assert out_vis[0, 3] == f32(1e30)  # (cr = 1e30, ci = 0: only p overflows)


# ------------------------------------------------------------------------------- errors
def test_host_errors():
    for bad in (0, 256, -1):
        with pytest.raises(ValueError, match="flag_value"):
            host.ApplyGainsHost(bad)
    for bad in (1.0, True, "1"):
        with pytest.raises(TypeError, match="flag_value"):
            host.ApplyGainsHost(bad)
    assert host.ApplyGainsHost().flag_value == 128 and host.ApplyGainsHost(255).flag_value == 255
    fn = host.ApplyGainsHost()
    good = gen.make_case(1, 4, 6, 3)
    fn(**good)
    bads = {
        "vis": [good["vis"].astype(np.complex128), good["vis"][0], np.zeros((0, 6), np.complex64),
                np.zeros((4, 0), np.complex64)],
        "gains": [good["gains"].astype(np.complex128), good["gains"][:3], good["gains"][0],
                  np.zeros((4, 0), np.complex64), np.zeros((4, 4097), np.complex64)],
        "inputs": [good["inputs"].astype(np.int64), good["inputs"][:5], good["inputs"].T,
                   good["inputs"][:, 0]],
        "weights": [good["weights"].astype(np.float64), good["weights"][:, :5], good["weights"][0]],
        "flags": [good["flags"].astype(np.int8), good["flags"][:3], good["flags"][0]],
    }  # fmt: skip
    for name, values in bads.items():
        for bad in values:
            with pytest.raises(ValueError, match=name):
                fn(**{**good, name: bad})
    fn(good["vis"], np.zeros((4, 4096), np.complex64), good["inputs"])


def test_template_and_operation_errors(context, queue):
    with pytest.raises(ValueError):
        ingest.ApplyGainsTemplate(context, tuning={"wgs": 256})
    assert ingest.ApplyGainsTemplate(context, tuning={}).tuning == {}
    assert ingest.ApplyGainsTemplate.autotune(context) == {}
    assert ingest.ApplyGainsTemplate.host_class is host.ApplyGainsHost
    assert ingest.ApplyGainsTemplate.KERNEL == "ksp_apply_gains"
    assert ingest.ApplyGainsTemplate.operation_class is ingest.ApplyGains
    for bad in (0, 256, -128):
        with pytest.raises(ValueError, match="flag_value"):
            ingest.ApplyGainsTemplate(context, flag_value=bad)
    with pytest.raises(TypeError, match="flag_value"):
        ingest.ApplyGainsTemplate(context, flag_value=1.5)
    template = ingest.ApplyGainsTemplate(context)
    assert template.kernel.name == "ksp_apply_gains"
    assert (template.weights, template.flags, template.flag_value) == (True, True, 128)
    for args in [(0, 4, 2), (4, 0, 2), (-4, 4, 2), (4, -1, 2), (4, 4, 0), (4, 4, -1), (4, 4, 4097)]:
        with pytest.raises(ValueError):
            template.instantiate(queue, *args)
    assert isinstance(template.instantiate(queue, 4, 5, 4096), ingest.ApplyGains)
    fn = template.instantiate(queue, 1, 1, 1)
    assert isinstance(fn, ingest.ApplyGains)
    assert fn.parameters() == {"weights": True, "flags": True, "flag_value": 128, "n_inputs": 1,
                               "channels": 1, "baselines": 1}  # fmt: skip


def test_host_from_device(context, queue):
    case = gen.make_case(1, 4, 5, 3)
    vis, gains, inputs = case["vis"], case["gains"], case["inputs"]
    for weights, flags in VARIANTS:
        template = ingest.ApplyGainsTemplate(context, weights=weights, flags=flags)
        adapter = ingest.ApplyGainsHostFromDevice(template, queue)
        given = {"weights": case["weights"] if weights else None,
                 "flags": case["flags"] if flags else None}  # fmt: skip
        del queue.launches[:]
        out = adapter(vis, gains, inputs, **given)
        assert (out[0].shape, out[0].dtype) == ((4, 5), np.complex64)
        assert (out[1] is not None) == weights and (out[2] is not None) == flags
        if weights:
            assert (out[1].shape, out[1].dtype) == ((4, 5), f32)
        if flags:
            assert (out[2].shape, out[2].dtype) == ((4, 5), np.uint8)
        assert [name for name, _ in queue.launches] == ["ksp_apply_gains"]
        assert [int(a) for a in queue.launches[0][1][8:11]] == [4, 5, 3]
        # each optional input exactly when the template has it
        for name in ("weights", "flags"):
            wrong = dict(given)
            wrong[name] = None if given[name] is not None else case[name]
            with pytest.raises(TypeError, match=name):
                adapter(vis, gains, inputs, **wrong)
    adapter = ingest.ApplyGainsHostFromDevice(ingest.ApplyGainsTemplate(context, False, False), queue)
    with pytest.raises(ValueError):
        adapter(vis[0], gains, inputs)
    with pytest.raises(ValueError):
        adapter(vis, np.zeros((4, 4097), np.complex64), inputs)
    with pytest.raises(ValueError):
        adapter(np.zeros((0, 5), np.complex64), gains[:0], inputs)


# ------------------------------------------------------------------------------- wiring
def expected_slots(weights, flags):
    names = ["vis", "out_vis"]
    names += ["weights", "out_weights"] if weights else []
    names += ["flags", "out_flags"] if flags else []
    return names + ["gains", "inputs"]


DTYPES = {"vis": np.complex64, "weights": np.float32, "flags": np.uint8}


@pytest.mark.parametrize("weights, flags", VARIANTS)
def test_slots(weights, flags, context, queue):
    template = ingest.ApplyGainsTemplate(context, weights=weights, flags=flags, flag_value=4)
    fn = template.instantiate(queue, 300, 200, 58)
    assert list(fn.slots) == expected_slots(weights, flags)
    for name, slot in fn.slots.items():
        if name == "gains":
            assert (slot.shape, slot.dtype) == ((300, 58), np.complex64)
        elif name == "inputs":
            assert (slot.shape, slot.dtype) == ((200, 2), np.int32)
            assert slot.dimensions[1].exact
        else:
            assert (slot.shape, slot.dtype) == ((300, 200), DTYPES[name.replace("out_", "")])
    # a dimension object of its own for everything that can be padded
    dims = [d for slot in fn.slots.values() for d in slot.dimensions]
    assert len({id(d) for d in dims}) == len(dims) == 2 * len(fn.slots)
    assert fn.parameters() == {"weights": weights, "flags": flags, "flag_value": 4,
                               "n_inputs": 58, "channels": 300, "baselines": 200}  # fmt: skip


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("weights, flags", VARIANTS)
def test_launch_arguments(weights, flags, in_place, context, queue):
    template = ingest.ApplyGainsTemplate(context, weights=weights, flags=flags, flag_value=32)
    fn = template.instantiate(queue, 300, 200, 58)
    kinds = ["vis"] + (["weights"] if weights else []) + (["flags"] if flags else [])
    if in_place:
        # one padded size per pair, larger than either asks for
        for kind in kinds:
            accel.Dimension(200, min_padded_size=500).link(fn.slots[kind].dimensions[1])
            fn.slots[kind].dimensions[1].link(fn.slots["out_" + kind].dimensions[1])
        fn.ensure_all_bound()
        fn.bind(**{"out_" + kind: fn.buffer(kind) for kind in kinds})
    else:
        accel.Dimension(200, min_padded_size=500).link(fn.slots["out_vis"].dimensions[1])
    fn()
    assert [name for name, _ in queue.launches] == ["ksp_apply_gains"]
    args = queue.launches[0][1]
    assert len(args) == 19

    def buf(name, present=True):
        return fn.buffer(name).buffer if present else None

    pointers = [buf("vis"), buf("weights", weights), buf("flags", flags), buf("gains"),
                buf("inputs"), buf("out_vis"), buf("out_weights", weights),
                buf("out_flags", flags)]  # fmt: skip
    for got, want in zip(args[:8], pointers):
        assert got is want
    for kind in kinds:
        assert (fn.buffer(kind) is fn.buffer("out_" + kind)) == in_place
    assert all(isinstance(a, np.int32) for a in args[8:])
    assert [int(a) for a in args[8:11]] == [300, 200, 58]

    def stride(name, present=True):
        return fn.buffer(name).padded_shape[1] if present else 0

    strides = [stride("vis"), stride("weights", weights), stride("flags", flags), stride("gains"),
               stride("out_vis"), stride("out_weights", weights), stride("out_flags", flags)]  # fmt: skip
    assert [int(a) for a in args[11:18]] == strides
    if in_place:  # 500 rounded up to whole 128-byte rows
        want = [512, 512 if weights else 0, 512 if flags else 0, 64] * 2
        assert strides == want[:4] + want[:3]
    else:
        assert strides == [208, 224 if weights else 0, 256 if flags else 0, 64, 512,
                           224 if weights else 0, 256 if flags else 0]  # fmt: skip
    assert int(args[18]) == 32
    assert fn.buffer("inputs").padded_shape[1] == 2


def test_between_finalise_and_compress(context, queue):
    """finalise -> apply_gains -> compress: the averaged arrays are `vis`, `weights` and `flags`
    of apply_gains, each one buffer with one padded size, and `out_weights` is compress's
    `weights`; the raw averaged output stays untouched in buffers of its own."""
    channels, baselines, cf, n_inputs = 4096, 200, 8, 64
    rows = channels // cf
    finalise = device.FinaliseTemplate(context, channel_factor=cf).instantiate(
        queue, channels, baselines)  # fmt: skip
    apply_gains = ingest.ApplyGainsTemplate(context).instantiate(queue, rows, baselines, n_inputs)
    compress = ingest.CompressWeightsTemplate(context).instantiate(queue, rows, baselines)
    # more row padding than any of them asks for, asked of one member of each compound
    accel.Dimension(baselines, min_padded_size=300).link(finalise.slots["weights"].dimensions[1])
    accel.Dimension(baselines, min_padded_size=700).link(compress.slots["weights"].dimensions[1])
    seq = accel.OperationSequence(
        queue, [("finalise", finalise), ("apply_gains", apply_gains), ("compress", compress)],
        compounds={"vis": ["finalise:vis", "apply_gains:vis"],
                   "weights": ["finalise:weights", "apply_gains:weights"],
                   "flags": ["finalise:flags", "apply_gains:flags"],
                   "cal_weights": ["apply_gains:out_weights", "compress:weights"]})  # fmt: skip
    assert {"vis", "weights", "flags", "cal_weights", "apply_gains:out_vis",
            "apply_gains:out_flags", "apply_gains:gains", "apply_gains:inputs",
            "compress:weights8"} <= set(seq.slots)  # fmt: skip
    seq()
    assert [name for name, _ in queue.launches] == [
        "ksp_average_finalise", "ksp_apply_gains", "ksp_compress_weights"]  # fmt: skip
    final_args, gains_args, compress_args = (launch[1] for launch in queue.launches)
    assert final_args[3] is gains_args[0] is seq.buffer("vis").buffer
    assert final_args[4] is gains_args[1] is seq.buffer("weights").buffer
    assert final_args[5] is gains_args[2] is seq.buffer("flags").buffer
    assert gains_args[6] is compress_args[0] is seq.buffer("cal_weights").buffer
    assert gains_args[5] is seq.buffer("apply_gains:out_vis").buffer
    assert len({id(a) for a in gains_args[:8]}) == 8  # out of place: eight buffers
    assert int(final_args[14]) == int(gains_args[12]) == seq.buffer("weights").padded_shape[1] == 320
    assert int(final_args[13]) == int(gains_args[11]) == seq.buffer("vis").padded_shape[1]
    assert int(final_args[15]) == int(gains_args[13]) == seq.buffer("flags").padded_shape[1]
    assert int(gains_args[16]) == int(compress_args[5]) == 704
    assert [int(a) for a in gains_args[8:11]] == [rows, baselines, n_inputs]


def test_in_place_behind_finalise(context, queue):
    """Each pair in one compound with finalise's output: the gains are applied in place."""
    finalise = device.FinaliseTemplate(context, channel_factor=4).instantiate(queue, 64, 40)
    apply_gains = ingest.ApplyGainsTemplate(context).instantiate(queue, 16, 40, 9)
    kinds = ("vis", "weights", "flags")
    seq = accel.OperationSequence(
        queue, [("finalise", finalise), ("apply_gains", apply_gains)],
        compounds={kind: ["finalise:" + kind, "apply_gains:" + kind, "apply_gains:out_" + kind]
                   for kind in kinds})  # fmt: skip
    seq()
    final_args, gains_args = (launch[1] for launch in queue.launches)
    for i, kind in enumerate(kinds):
        assert final_args[3 + i] is gains_args[i] is gains_args[5 + i] is seq.buffer(kind).buffer
        assert int(gains_args[11 + i]) == int(gains_args[15 + i]) == seq.buffer(kind).padded_shape[1]


# ------------------------------------------------------------------- the launcher's checks
@pytest.fixture(scope="module")
def lib():
    from katsdpsigproc_amd import _lib, build_native

    if not os.path.exists(_lib.LIB_PATH):
        build_native.build()
    return _lib.load()


def test_argument_validation_without_gpu(lib):
    from katsdpsigproc_amd import _lib

    # never dereferenced: every call below fails its checks first. Eight arrays far apart.
    p = {name: ctypes.c_void_p((i + 1) << 32) for i, name in enumerate(
        ["vis", "weights", "flags", "gains", "inputs", "out_vis", "out_weights", "out_flags"])}

    def call(channels=4, baselines=8, n_inputs=3, flag_value=128, **changed):
        a = dict(p, vis_stride=8, weights_stride=8, flags_stride=8, gains_stride=3,
                 out_vis_stride=8, out_weights_stride=8, out_flags_stride=8)  # fmt: skip
        a.update(changed)
        rc = lib.ksp_apply_gains(
            0, None, a["vis"], a["weights"], a["flags"], a["gains"], a["inputs"], a["out_vis"],
            a["out_weights"], a["out_flags"], channels, baselines, n_inputs, a["vis_stride"],
            a["weights_stride"], a["flags_stride"], a["gains_stride"], a["out_vis_stride"],
            a["out_weights_stride"], a["out_flags_stride"], flag_value)  # fmt: skip
        assert rc != 0
        return _lib.last_error()

    for name in ("vis", "gains", "inputs", "out_vis"):
        assert f"invalid argument: {name} is NULL" in call(**{name: None})
    for name in ("weights", "out_weights"):
        assert "weights and out_weights must both be NULL or both be given" in call(**{name: None})
    for name in ("flags", "out_flags"):
        assert "flags and out_flags must both be NULL or both be given" in call(**{name: None})
    for bad in (0, -1):
        assert "invalid argument: channels must be at least 1" in call(channels=bad)
        assert "invalid argument: baselines must be at least 1" in call(baselines=bad)
    for bad in (0, -1, 4097):
        assert "invalid argument: n_inputs must be 1..4096" in call(n_inputs=bad, gains_stride=4097)
    for bad in (0, 256, -128):
        assert "invalid argument: flag_value must be 1..255" in call(flag_value=bad)
    for name in ("vis", "weights", "flags", "out_vis", "out_weights", "out_flags"):
        assert f"invalid argument: {name}_stride is smaller than baselines" in call(
            **{name + "_stride": 7})
    assert "invalid argument: gains_stride is smaller than n_inputs" in call(gains_stride=2)
    assert "gains_stride is smaller" in call(n_inputs=4096, gains_stride=4095)
    # the order of the checks: everything wrong at once, then only every stride
    strides = {name + "_stride": -1 for name in (
        "vis", "weights", "flags", "gains", "out_vis", "out_weights", "out_flags")}  # fmt: skip
    assert "invalid argument: vis is NULL" in call(
        channels=0, baselines=0, n_inputs=0, flag_value=0, **dict.fromkeys(p), **strides)
    assert "invalid argument: vis_stride is smaller than baselines" in call(**strides)
    assert "invalid argument: gains_stride is smaller than n_inputs" in call(
        **dict(strides, vis_stride=8, out_vis_stride=8))  # fmt: skip
    # an absent pair's strides are not looked at: the call gets as far as the next check
    none_w = dict(weights=None, out_weights=None, weights_stride=0, out_weights_stride=0)
    none_f = dict(flags=None, out_flags=None, flags_stride=0, out_flags_stride=0)
    assert "flag_value must be 1..255" not in call(**none_w, vis_stride=7)
    assert "vis_stride is smaller" in call(**none_w, **none_f, vis_stride=7)

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
        # in place, and arrays that only touch, pass this check: the next failure is reported
        for fine in (p[kind], at(kind, extent), at(kind, -extent)):
            assert "invalid argument: n_inputs" in call(**{out: fine}, n_inputs=0)
        # a pair that is absent is not compared
    assert "n_inputs" in call(**none_w, **none_f, n_inputs=0)


def test_header_binding_and_exports_agree(lib):
    from katsdpsigproc_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "katsdpsigproc_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declaration = re.search(r"int ksp_apply_gains\((.*?)\);", text, re.S)
    assert declaration is not None
    parameters = [" ".join(part.split()) for part in declaration.group(1).split(",")]
    argtypes = _lib.SIGNATURES["ksp_apply_gains"]
    assert len(parameters) == len(argtypes) == 21
    for parameter, argtype in zip(parameters, argtypes):
        assert ("*" in parameter) == (argtype is ctypes.c_void_p), parameter
        assert argtype in (ctypes.c_int, ctypes.c_void_p)
    names = [parameter.replace("*", " ").split()[-1] for parameter in parameters]
    assert names == ["device", "stream", "vis", "weights", "flags", "gains", "inputs", "out_vis",
                     "out_weights", "out_flags", "channels", "baselines", "n_inputs", "vis_stride",
                     "weights_stride", "flags_stride", "gains_stride", "out_vis_stride",
                     "out_weights_stride", "out_flags_stride", "flag_value"]  # fmt: skip
    assert hasattr(lib, "ksp_apply_gains")
    assert lib.ksp_abi_version() == _lib.ABI_VERSION == 5
    for name in ("ApplyGainsTemplate", "ApplyGains", "ApplyGainsHostFromDevice"):
        assert hasattr(ingest, name)
    assert hasattr(host, "ApplyGainsHost")
