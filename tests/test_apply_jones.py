"""Applying Jones matrices without a GPU: ``rfi.host.ApplyJonesHost`` against a loop of float32
scalars and known answers, ``quad_table``, ``ApplyGainsHost`` on diagonal matrices, the model
data of the solver, argument errors, slot lists and every launch argument of every variant on
the fake backend, the sequence finalise -> solve_jones -> apply_jones -> compress, and the
argument checks of ``ksp_apply_jones``, which come before any device call."""

import ctypes
import os
import re

import numpy as np
import pytest

from katsdpsigproc_amd import accel
from katsdpsigproc_amd.rfi import device, host, ingest
from tests import inputs_apply_jones as gen
from tests import inputs_solve_jones
from tests.fakes import FakeContext
from tests.inputs_apply_jones import assert_same

f32 = np.float32
VARIANTS = [(True, True), (True, False), (False, True), (False, False)]
KINDS = ("vis", "weights", "flags")


@pytest.fixture
def context():
    return FakeContext()


@pytest.fixture
def queue(context):
    return context.create_command_queue()


def arguments(case, weights=True, flags=True):
    return (case["vis"], case["jones"], case["quad_antennas"], case["quads"],
            case["weights"] if weights else None, case["flags"] if flags else None)  # fmt: skip


# ------------------------------------------------------------------------- the scalar loop
def cmul(a, b):
    return (f32(f32(a[0] * b[0]) - f32(a[1] * b[1])), f32(f32(a[0] * b[1]) + f32(a[1] * b[0])))


def cmul_conj(a, b):
    return (f32(f32(a[0] * b[0]) + f32(a[1] * b[1])), f32(f32(a[1] * b[0]) - f32(a[0] * b[1])))


def cadd(a, b):
    return (f32(a[0] + b[0]), f32(a[1] + b[1]))


def norm2(a):
    return f32(f32(a[0] * a[0]) + f32(a[1] * a[1]))


def scalar_loop(vis, jones, quad_antennas, quads, weights, flags, flag_value):
    """The definition, quad by quad and step by step, in np.float32 scalars. The outputs start
    as the inputs: a baseline in no quad keeps them."""
    channels, baselines = vis.shape
    n_ant = jones.shape[1] // 2
    out_vis, out_weights, out_flags = vis.copy(), weights.copy(), flags.copy()

    def parts(z):
        return (f32(z.real), f32(z.imag))

    with np.errstate(all="ignore"):
        for c in range(channels):
            for (a, b), entries in zip(quad_antennas.tolist(), quads.tolist()):
                present = [t != 0 and abs(t) <= baselines for t in entries]
                where = [abs(t) - 1 if p else None for t, p in zip(entries, present)]
                s, w, have, any_f = [None] * 4, [f32(1)] * 4, list(present), 0
                for e in range(4):
                    if present[e]:
                        re, im = parts(vis[c, where[e]])
                        s[e] = (re, -im if entries[e] < 0 else im)
                        w[e] = weights[c, where[e]]
                        any_f |= int(flags[c, where[e]])
                if a == b:
                    for e, other in ((1, 2), (2, 1)):
                        if not present[e] and present[other]:
                            s[e], w[e], have[e] = (s[other][0], -s[other][1]), w[other], True
                ok = 0 <= a < n_ant and 0 <= b < n_ant and all(have)
                if ok:
                    ca = [[parts(jones[c, 2 * a + i, m]) for m in range(2)] for i in range(2)]
                    cb = [[parts(jones[c, 2 * b + k, n]) for n in range(2)] for k in range(2)]
                    ok = not any(np.isnan(x) for mat in (ca, cb) for row in mat for z in row
                                 for x in z)  # fmt: skip
                for e in range(4):
                    if not present[e]:
                        continue
                    i, k = divmod(e, 2)
                    j = where[e]
                    out_flags[c, j] = any_f | (0 if ok else flag_value)
                    out_weights[c, j] = 0
                    if not ok:
                        continue
                    t0 = cadd(cmul(ca[i][0], s[0]), cmul(ca[i][1], s[2]))
                    t1 = cadd(cmul(ca[i][0], s[1]), cmul(ca[i][1], s[3]))
                    o = cadd(cmul_conj(t0, cb[k][0]), cmul_conj(t1, cb[k][1]))
                    out_vis[c, j] = complex(o[0], -o[1] if entries[e] < 0 else o[1])
                    if all(x > 0 for x in w):
                        r = [f32(f32(1) / x) for x in w]
                        u0 = f32(f32(norm2(ca[i][0]) * r[0]) + f32(norm2(ca[i][1]) * r[2]))
                        u1 = f32(f32(norm2(ca[i][0]) * r[1]) + f32(norm2(ca[i][1]) * r[3]))
                        var = f32(f32(u0 * norm2(cb[k][0])) + f32(u1 * norm2(cb[k][1])))
                        if var > 0:
                            out_weights[c, j] = f32(f32(1) / var)
    return out_vis, out_weights, out_flags


@pytest.mark.parametrize("order", gen.ORDERS)
@pytest.mark.parametrize("dish", gen.DISHES)
def test_host_against_the_scalar_loop(order, dish):
    for n_ant, spoil in ((1, False), (3, True), (4, False), (17, True)):
        channels = 3 if n_ant == 17 else 7
        case = gen.make_case(n_ant + 3, channels, n_ant, order, dish, spoil=spoil, extra=2, flag_value=4)
        want = scalar_loop(*arguments(case), 4)
        got = host.ApplyJonesHost(4)(*arguments(case))
        for name, w, g in zip(KINDS, want, got):
            assert_same(w, g, f"out_{name}, {n_ant} antennas")
        plain = host.ApplyJonesHost(4)(*arguments(case, False, False))
        assert plain[1] is None and plain[2] is None
        assert_same(want[0], plain[0], "out_vis alone")


def test_host_modifies_no_argument():
    case = gen.make_case(1, 4, 3, "random", "one", spoil=True)
    before = [x.copy() for x in arguments(case)]
    host.ApplyJonesHost()(*arguments(case))
    for x, y in zip(before, arguments(case)):
        assert (x.view(np.uint8) == y.view(np.uint8)).all()


# -------------------------------------------------------------------------------- the table
@pytest.mark.parametrize("order", gen.ORDERS)
@pytest.mark.parametrize("dish", gen.DISHES)
@pytest.mark.parametrize("n_ant", gen.ANTENNAS)
def test_quad_table(n_ant, dish, order):
    inputs = gen.make_inputs(n_ant, n_ant, order, dish)
    inputs = np.concatenate([inputs, [(-1, 0), (0, 2 * n_ant), (2 * n_ant, 2 * n_ant)]]).astype(np.int32)
    quad_antennas, quads = host.ApplyJonesHost.quad_table(inputs, 2 * n_ant)
    assert quad_antennas.dtype == quads.dtype == np.int32
    assert quad_antennas.shape == (gen.n_quads_of(n_ant), 2) and quads.shape == (len(quads), 4)
    assert (quad_antennas[:, 0] <= quad_antennas[:, 1]).all()
    assert len({tuple(row) for row in quad_antennas.tolist()}) == len(quads)
    # every baseline between known inputs in exactly one entry, the others in none
    named = np.abs(quads[quads != 0]) - 1
    assert sorted(named.tolist()) == list(range(len(inputs) - 3))
    for (a, b), row in zip(quad_antennas.tolist(), quads.tolist()):
        for entry, t in enumerate(row):
            if t == 0:
                assert a == b and entry in (1, 2) and dish != "both"
                continue
            p, q = 2 * a + entry // 2, 2 * b + entry % 2
            assert tuple(inputs[abs(t) - 1]) == ((p, q) if t > 0 else (q, p))
            assert t > 0 or a < b
    # ordered by the smallest baseline a quad names
    first = [min(abs(t) for t in row if t) for row in quads.tolist()]
    assert first == sorted(first)
    if order != "random":  # neighbouring quads are neighbouring baselines
        assert first == list(range(1, len(first) + 1)) or order == "adjacent"
    assert gen.covered(quads, len(inputs)).tolist() == [True] * (len(inputs) - 3) + [False] * 3


def test_quad_table_errors():
    table = host.ApplyJonesHost.quad_table
    with pytest.raises(ValueError, match=r"inputs lists the pair \(2, 5\) twice: baselines 1 and 3"):
        table([(0, 0), (2, 5), (1, 1), (2, 5)], 6)
    with pytest.raises(ValueError, match=r"inputs lists the pair \(2, 5\) twice: baselines 0 and 1"):
        table([(2, 5), (5, 2)], 6)
    with pytest.raises(ValueError, match=r"inputs lists the pair \(3, 3\) twice"):
        table([(3, 3), (3, 3)], 4)
    table([(2, 3), (3, 2)], 4)  # the two cross hands of a dish are two baselines
    for nothing in ([(-1, 0), (0, 4), (7, 7)], np.zeros((0, 2), np.int32)):
        with pytest.raises(ValueError, match="no baseline"):
            table(nothing, 4)
    for bad in (0, 1, 3, 2049, 2050, -2):
        with pytest.raises(ValueError, match=r"n_inputs must be even and 2\.\.2048"):
            table([(0, 0)], bad)
    with pytest.raises(TypeError, match="n_inputs"):
        table([(0, 0)], 4.0)
    for bad in (np.zeros((3, 3), np.int32), np.zeros(4, np.int32), np.zeros((3, 2), f32)):
        with pytest.raises(ValueError, match="inputs must be integers"):
            table(bad, 4)
    assert host.ApplyJonesHost.check_n_inputs(np.int64(2048)) == 2048


# ---------------------------------------------------------------------------- known answers
def identity_jones(channels, n_inputs):
    jones = np.zeros((channels, n_inputs, 2), np.complex64)
    jones[:, 0::2, 0] = 1
    jones[:, 1::2, 1] = 1
    return jones


def clean_case(seed, channels, n_ant, order="random", dish="one"):
    """Finite data, positive weights, no flags, identity matrices."""
    rs = np.random.RandomState(seed)
    inputs = gen.make_inputs(seed, n_ant, order, dish)
    quad_antennas, quads = host.ApplyJonesHost.quad_table(inputs, 2 * n_ant)
    shape = (channels, len(inputs))
    vis = (rs.standard_normal(shape) + 1j * rs.standard_normal(shape)).astype(np.complex64)
    return {"vis": vis, "jones": identity_jones(channels, 2 * n_ant), "inputs": inputs,
            "quad_antennas": quad_antennas, "quads": quads,
            "weights": rs.uniform(0.5, 2, shape).astype(f32),
            "flags": np.zeros(shape, np.uint8)}  # fmt: skip


def test_identity_leaves_vis_equal():
    case = clean_case(1, 5, 4)
    out_vis, out_weights, out_flags = host.ApplyJonesHost()(*arguments(case))
    assert (out_vis == case["vis"]).all()  # (as numbers: a zero may change its sign)
    assert not out_flags.any()
    # var = 1 / w of the sample itself: 1 / (1 / w) is w to one rounding each way
    assert np.allclose(out_weights, case["weights"], rtol=3e-7, atol=0)


def test_flags_are_ored_over_the_quad():
    case = clean_case(2, 3, 3, "blocks", "both")
    quads = case["quads"]
    for q, bit in ((0, 1), (2, 2), (4, 0x80)):
        case["flags"][1, abs(quads[q, q % 4]) - 1] = bit
    out_flags = host.ApplyJonesHost(0x80)(*arguments(case))[2]
    want = np.zeros_like(out_flags)
    for q, bit in ((0, 1), (2, 2), (4, 0x80)):
        want[1, np.abs(quads[q]) - 1] = bit
    assert (out_flags == want).all()
    # a weight that is not positive takes the weights of all four, and no flag
    for bad in (0.0, -1.0, np.nan):
        case["weights"][2, abs(quads[1, 3]) - 1] = bad
        _, out_weights, again = host.ApplyJonesHost(0x80)(*arguments(case))
        assert not out_weights[2, np.abs(quads[1]) - 1].any() and (again == want).all()
        assert (out_weights[2, np.abs(quads[0]) - 1] > 0).all()


def test_incomplete_quads_and_bad_antennas_pass_through():
    case = clean_case(3, 4, 3, "random", "both")
    case["jones"] = gen.make_jones(3, 4, 6, special=False, span=2)
    baselines = case["vis"].shape[1]
    quads, ants = case["quads"], case["quad_antennas"]
    # two quads between dishes (within a dish a missing cross hand has a stand-in)
    q, other = np.flatnonzero(ants[:, 0] != ants[:, 1])[:2]
    dropped = abs(int(quads[q, 2])) - 1
    for junk in (0, baselines + 1, -(baselines + 1), gen.INT32_MIN, gen.INT32_MAX):
        quads[q, 2] = junk
        out = host.ApplyJonesHost(0x10)(*arguments(case))
        rest = np.abs(quads[q, [0, 1, 3]]) - 1
        assert (out[0][:, rest] == case["vis"][:, rest]).all()
        assert not out[1][:, rest].any() and (out[2][:, rest] == 0x10).all()
        # the baseline that left the table is in no quad: its outputs are its inputs
        for got, given in zip(out, arguments(case)[:1] + arguments(case)[4:]):
            assert (got[:, dropped] == given[:, dropped]).all()
        fine = np.abs(quads[other]) - 1
        assert (out[0][:, fine] != case["vis"][:, fine]).all() and not out[2][:, fine].any()
    for bad in (-1, 3, gen.INT32_MIN, gen.INT32_MAX):
        for side in (0, 1):
            changed = ants.copy()
            changed[other, side] = bad
            out = host.ApplyJonesHost(0x10)(case["vis"], case["jones"], changed, quads,
                                            case["weights"], case["flags"])  # fmt: skip
            there = np.abs(quads[other]) - 1
            assert (out[0][:, there] == case["vis"][:, there]).all()
            assert not out[1][:, there].any() and (out[2][:, there] == 0x10).all()


def test_a_nan_in_each_of_the_sixteen_floats():
    case = clean_case(4, 2, 2, "adjacent", "both")
    case["jones"] = gen.make_jones(4, 2, 4, special=False, span=2)
    quad = [tuple(row) for row in case["quad_antennas"].tolist()].index((0, 1))
    there = np.abs(case["quads"][quad]) - 1
    clean = host.ApplyJonesHost()(*arguments(case))
    assert not clean[2].any()
    for part in range(16):
        jones = case["jones"].copy()
        jones[1].view(f32).reshape(-1)[part] = np.nan  # rows 0..3 of channel 1: 16 floats
        out = host.ApplyJonesHost()(case["vis"], jones, *arguments(case)[2:])
        assert (out[0][1, there] == case["vis"][1, there]).all()
        assert not out[1][1, there].any() and (out[2][1, there] == 128).all()
        for got, want in zip(out, clean):  # the other channel is as it was
            assert_same(want[0], got[0], f"part {part}")
        # each dish's own quad is touched exactly when the NaN is in its matrix
        for dish in (0, 1):
            own = [tuple(row) for row in case["quad_antennas"].tolist()].index((dish, dish))
            at = np.abs(case["quads"][own]) - 1
            assert (out[2][1, at] == 128).all() == (part // 8 == dish)


def test_the_hermitian_stand_in():
    """(2a, 2a+1) alone, (2a+1, 2a) alone and both with conjugate data give the same answers."""
    both = clean_case(5, 3, 2, "adjacent", "both")
    both["jones"] = gen.make_jones(5, 3, 4, special=False, span=2)
    both["flags"][...] = np.random.RandomState(5).randint(0, 4, both["flags"].shape)
    inputs = both["inputs"]
    pair = {(int(p), int(q)): j for j, (p, q) in enumerate(inputs.tolist())}
    for a in (0, 1):  # make the second cross hand the conjugate of the first
        j, mirror = pair[(2 * a, 2 * a + 1)], pair[(2 * a + 1, 2 * a)]
        both["vis"][:, mirror] = np.conj(both["vis"][:, j])
        both["weights"][:, mirror] = both["weights"][:, j]
        both["flags"][:, mirror] = both["flags"][:, j]
    full = host.ApplyJonesHost()(*arguments(both))
    for keep in (0, 1):
        drop = [pair[(2 * a + 1 - keep, 2 * a + keep)] for a in (0, 1)]
        quads = both["quads"].copy()
        quads[np.isin(np.abs(quads) - 1, drop)] = 0
        assert (quads == 0).sum() == 2
        out = host.ApplyJonesHost()(both["vis"], both["jones"], both["quad_antennas"], quads,
                                    both["weights"], both["flags"])  # fmt: skip
        rest = np.setdiff1d(np.arange(len(inputs)), drop)
        for name, w, g, given in zip(KINDS, full, out, (both["vis"], both["weights"], both["flags"])):
            assert_same(np.ascontiguousarray(w[:, rest]), np.ascontiguousarray(g[:, rest]), name)
            assert (g[:, drop] == given[:, drop]).all()  # nothing is stored for the absent entry
        assert not (out[2] & 128).any()
    # with neither cross hand the dish's quad is incomplete
    quads = both["quads"].copy()
    quads[np.isin(np.abs(quads) - 1, [pair[(0, 1)], pair[(1, 0)]])] = 0
    out = host.ApplyJonesHost()(both["vis"], both["jones"], both["quad_antennas"], quads,
                                both["weights"], both["flags"])  # fmt: skip
    assert (out[2][:, [pair[(0, 0)], pair[(1, 1)]]] & 128).all()
    assert not (out[2][:, [pair[(2, 2)], pair[(3, 3)], pair[(0, 2)]]] & 128).any()


def test_uncovered_baselines_keep_their_values():
    case = gen.make_case(6, 5, 4, "random", "one", extra=4)
    out = host.ApplyJonesHost()(*arguments(case))
    for got, given in zip(out, (case["vis"], case["weights"], case["flags"])):
        assert (got[:, -4:].view(np.uint8) == given[:, -4:].view(np.uint8)).all()
    assert not gen.covered(case["quads"], case["vis"].shape[1])[-4:].any()


# ------------------------------------------------------------------------ against ApplyGains
def test_diagonal_matrices_against_apply_gains():
    """C_a = diag(g_2a, g_2a+1) on complete quads with finite data is ApplyGainsHost: each
    path is two complex products of about 6 roundings of 2^-24 |g_a||g_b||v| per part (16
    asserted), and a weight is at most 16 roundings away (1e-6 asserted)."""
    worst_vis = worst_w = 0.0
    for seed, n_ant, order in ((1, 3, "blocks"), (2, 4, "adjacent"), (3, 17, "random")):
        case = clean_case(seed, 6, n_ant, order, "both")
        rs = np.random.RandomState(seed + 50)
        shape = (6, 2 * n_ant)
        gains = (np.exp2(rs.uniform(-3, 3, shape)) * np.exp(2j * np.pi * rs.random_sample(shape)))
        gains = gains.astype(np.complex64)
        jones = np.zeros(shape + (2,), np.complex64)
        jones[:, 0::2, 0] = gains[:, 0::2]
        jones[:, 1::2, 1] = gains[:, 1::2]
        case["flags"][...] = rs.randint(0, 2, case["flags"].shape) * (rs.random_sample(case["flags"].shape) < 0.05)
        ours = host.ApplyJonesHost()(case["vis"], jones, *arguments(case)[2:])
        theirs = host.ApplyGainsHost()(case["vis"], gains, case["inputs"], case["weights"], case["flags"])
        a, b = case["inputs"][:, 0], case["inputs"][:, 1]
        scale = (np.abs(gains[:, a]).astype(np.float64) * np.abs(gains[:, b]) * np.abs(case["vis"]))
        unit = 2.0**-24 * scale
        diff = ours[0].astype(np.complex128) - theirs[0].astype(np.complex128)
        worst_vis = max(worst_vis, float((np.abs(diff.real) / unit).max()),
                        float((np.abs(diff.imag) / unit).max()))  # fmt: skip
        assert (theirs[1] > 0).all() and (ours[1] > 0).all()
        worst_w = max(worst_w, float(np.abs(ours[1].astype(np.float64) / theirs[1] - 1).max()))
        assert ((theirs[2] & ~ours[2]) == 0).all()  # the gains' flags are a subset
        assert (ours[2] != theirs[2]).any()  # (ours spread over the quad)
    print(f"diagonal matrices: vis within {worst_vis:.2f} units, weights within {worst_w:.2e}")
    assert worst_vis <= 16 and worst_w <= 1e-6


# -------------------------------------------------------------------- behind the solver
#: test_converges_to_the_true_products of tests/test_solve_jones.py: the solved products are
#: within this of the true ones, relative to the largest (the noise of the model data)
PRODUCT_ACCURACY = 2e-3
MODEL_NOISE = 0.01  # inputs_solve_jones.model_vis, per part


def test_behind_the_solver_on_model_data():
    """SolveJonesHost(corrections=True) -> ApplyJonesHost on the model data of
    tests/inputs_solve_jones.py: parallel hands 1 and cross hands 0. With C the inverse of the
    solved matrix, C_a (J^_a J^_b^H) C_b^H is the identity, so a calibrated sample is off by
    C_a (P - P^ + N) C_b^H: the error of the solved product (at most PRODUCT_ACCURACY times the
    largest product, the bound of the solver's own test on this case) plus the sample's noise
    (6 sigma of a Rayleigh deviate: 1e-8 of the samples lie beyond), each entry weighted by
    |C_a[i][m]| |C_b[k][n]|."""
    case = inputs_solve_jones.make_case(5, 4, 48, "missing", "clean")
    baselines = case["vis"].shape[1]
    jones, _, status = host.SolveJonesHost(200, 1e-6, corrections=True)(
        case["vis"], case["pairs"], case["weights"], case["flags"])  # fmt: skip
    assert not status.any()
    inputs = inputs_solve_jones.inputs_of(case["pairs"], baselines)
    inputs[(inputs == 0).all(axis=1)] = -1  # (what the table does not name is no baseline)
    quad_antennas, quads = host.ApplyJonesHost.quad_table(inputs, 48)
    out_vis, out_weights, out_flags = host.ApplyJonesHost()(
        case["vis"], jones, quad_antennas, quads, case["weights"], case["flags"])  # fmt: skip
    largest = np.abs(inputs_solve_jones.products(case["truth"])).max()
    slack = PRODUCT_ACCURACY * largest + 6 * MODEL_NOISE
    c = np.abs(jones.astype(np.complex128))  # (channels, n_inputs, 2)
    checked = 0
    for (a, b), row in zip(quad_antennas.tolist(), quads.tolist()):
        if a == b or 0 in row:
            continue
        for entry, t in enumerate(row):
            i, k = divmod(entry, 2)
            j = abs(t) - 1
            kept = out_flags[:, j] == 0
            bound = slack * c[:, 2 * a + i, :].sum(axis=1) * c[:, 2 * b + k, :].sum(axis=1)
            off = np.abs(out_vis[:, j].astype(np.complex128) - (1.0 if i == k else 0.0))
            assert (off[kept] <= bound[kept]).all(), (a, b, entry, off, bound)
            assert (out_weights[kept, j] > 0).all()
            checked += int(kept.sum())
    assert checked > 0.5 * 4 * 4 * 24 * 23 // 2


# ------------------------------------------------------------------------------- errors
def test_host_errors():
    for bad in (0, 256, -128):
        with pytest.raises(ValueError, match="flag_value"):
            host.ApplyJonesHost(bad)
    with pytest.raises(TypeError, match="flag_value"):
        host.ApplyJonesHost(1.5)
    assert host.ApplyJonesHost(255).flag_value == 255 and host.ApplyJonesHost().flag_value == 128
    assert host.ApplyJonesHost.MAX_INPUTS == 2048
    fn = host.ApplyJonesHost()
    case = gen.make_case(1, 4, 3, "random", "one")
    good = dict(zip(("vis", "jones", "quad_antennas", "quads", "weights", "flags"), arguments(case)))
    fn(**good)
    bads = {
        "vis": [good["vis"].astype(np.complex128), good["vis"][0], good["vis"][:, :0],
                good["vis"][:0]],
        "jones": [good["jones"].astype(np.complex128), good["jones"][:3], good["jones"][:, :, :1],
                  good["jones"][:, :5], good["jones"][:, :, 0], np.zeros((4, 0, 2), np.complex64),
                  np.zeros((4, 2050, 2), np.complex64)],
        "quad_antennas": [good["quad_antennas"].astype(np.int64), good["quad_antennas"][:, :1],
                          good["quad_antennas"][:0], good["quad_antennas"][0]],
        "quads": [good["quads"].astype(np.int64), good["quads"][:-1], good["quads"][:, :3],
                  good["quads"].T],
        "weights": [good["weights"].astype(np.float64), good["weights"][:, :5], good["weights"][0]],
        "flags": [good["flags"].astype(np.int8), good["flags"][:3], good["flags"][0]],
    }  # fmt: skip
    for name, values in bads.items():
        for bad in values:
            with pytest.raises(ValueError, match=name):
                fn(**{**good, name: bad})
    # one baseline in two present entries
    twice = good["quads"].copy()
    twice[1, 0] = -twice[0, 3]
    with pytest.raises(ValueError, match=f"quads names baseline {abs(int(twice[1, 0])) - 1} in more"):
        fn(**{**good, "quads": twice})
    fn(good["vis"], np.zeros((4, 2048, 2), np.complex64), good["quad_antennas"], good["quads"])


def test_template_and_operation_errors(context, queue):
    with pytest.raises(ValueError):
        ingest.ApplyJonesTemplate(context, tuning={"wgs": 256})
    assert ingest.ApplyJonesTemplate(context, tuning={}).tuning == {}
    assert ingest.ApplyJonesTemplate.autotune(context) == {}
    assert ingest.ApplyJonesTemplate.host_class is host.ApplyJonesHost
    assert ingest.ApplyJonesTemplate.KERNEL == "ksp_apply_jones"
    assert ingest.ApplyJonesTemplate.operation_class is ingest.ApplyJones
    for bad in (0, 256, -128):
        with pytest.raises(ValueError, match="flag_value"):
            ingest.ApplyJonesTemplate(context, flag_value=bad)
    with pytest.raises(TypeError, match="flag_value"):
        ingest.ApplyJonesTemplate(context, flag_value=1.5)
    template = ingest.ApplyJonesTemplate(context)
    assert template.kernel.name == "ksp_apply_jones"
    assert (template.weights, template.flags, template.flag_value) == (True, True, 128)
    for args in [(0, 4, 2, 1), (4, 0, 2, 1), (-4, 4, 2, 1), (4, -1, 2, 1), (4, 4, 0, 1),
                 (4, 4, 3, 1), (4, 4, -2, 1), (4, 4, 2050, 1), (4, 4, 2, 0), (4, 4, 2, -1)]:  # fmt: skip
        with pytest.raises(ValueError):
            template.instantiate(queue, *args)
    for args in [(4, 4, 2.0, 1), (4, 4, 2, 1.0), (4, 4, 2, True)]:
        with pytest.raises(TypeError):
            template.instantiate(queue, *args)
    assert isinstance(template.instantiate(queue, 4, 5, 2048, 7), ingest.ApplyJones)
    fn = template.instantiate(queue, 1, 1, 2, 1)
    assert fn.parameters() == {"weights": True, "flags": True, "flag_value": 128, "n_inputs": 2,
                               "n_quads": 1, "channels": 1, "baselines": 1}  # fmt: skip


def test_host_from_device(context, queue):
    case = gen.make_case(1, 4, 2, "random", "one", extra=1)
    vis, jones, inputs = case["vis"], case["jones"], case["inputs"]
    for weights, flags in VARIANTS:
        template = ingest.ApplyJonesTemplate(context, weights=weights, flags=flags)
        adapter = ingest.ApplyJonesHostFromDevice(template, queue)
        given = {"weights": case["weights"] if weights else None,
                 "flags": case["flags"] if flags else None}  # fmt: skip
        del queue.launches[:]
        out = adapter(vis, jones, inputs, **given)
        # the fake kernel does nothing: what comes back is what the outputs were filled with
        assert_same(vis, out[0], "out_vis starts as vis")
        assert (out[1] is not None) == weights and (out[2] is not None) == flags
        if weights:
            assert_same(case["weights"], out[1], "out_weights starts as weights")
        if flags:
            assert_same(case["flags"], out[2], "out_flags starts as flags")
        assert [name for name, _ in queue.launches] == ["ksp_apply_jones"]
        assert [int(a) for a in queue.launches[0][1][9:13]] == [4, len(inputs), 4, 3]
        for name in ("weights", "flags"):
            wrong = dict(given)
            wrong[name] = None if given[name] is not None else case[name]
            with pytest.raises(TypeError, match=name):
                adapter(vis, jones, inputs, **wrong)
    adapter = ingest.ApplyJonesHostFromDevice(ingest.ApplyJonesTemplate(context, False, False), queue)
    with pytest.raises(ValueError):
        adapter(vis[0], jones, inputs)
    with pytest.raises(ValueError, match="inputs"):
        adapter(vis, jones, inputs[:-1])
    with pytest.raises(ValueError, match="jones"):
        adapter(vis, jones[:, :, 0], inputs)
    with pytest.raises(ValueError, match="n_inputs"):
        adapter(vis, np.zeros((4, 2050, 2), np.complex64), inputs)
    with pytest.raises(ValueError, match="twice"):
        adapter(vis, jones, np.zeros_like(inputs))
    with pytest.raises(ValueError, match="no baseline"):
        adapter(vis, jones, np.full_like(inputs, 4))


# ------------------------------------------------------------------------------- wiring
def expected_slots(weights, flags):
    names = ["vis", "out_vis"]
    names += ["weights", "out_weights"] if weights else []
    names += ["flags", "out_flags"] if flags else []
    return names + ["jones", "quad_antennas", "quads"]


DTYPES = {"vis": np.complex64, "weights": np.float32, "flags": np.uint8}


@pytest.mark.parametrize("weights, flags", VARIANTS)
def test_slots(weights, flags, context, queue):
    template = ingest.ApplyJonesTemplate(context, weights=weights, flags=flags, flag_value=4)
    fn = template.instantiate(queue, 300, 200, 58, 77)
    assert list(fn.slots) == expected_slots(weights, flags)
    for name, slot in fn.slots.items():
        if name == "jones":
            assert (slot.shape, slot.dtype) == ((300, 58, 2), np.complex64)
            assert slot.dimensions[2].exact and not slot.dimensions[1].exact
        elif name in ("quad_antennas", "quads"):
            assert (slot.shape, slot.dtype) == ((77, 2 if name == "quad_antennas" else 4), np.int32)
            assert slot.dimensions[1].exact
        else:
            assert (slot.shape, slot.dtype) == ((300, 200), DTYPES[name.replace("out_", "")])
    # a dimension object of its own for everything that can be padded
    dims = [d for slot in fn.slots.values() for d in slot.dimensions]
    assert len({id(d) for d in dims}) == len(dims) == 2 * len(fn.slots) + 1
    assert fn.parameters() == {"weights": weights, "flags": flags, "flag_value": 4, "n_inputs": 58,
                               "n_quads": 77, "channels": 300, "baselines": 200}  # fmt: skip


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("weights, flags", VARIANTS)
def test_launch_arguments(weights, flags, in_place, context, queue):
    template = ingest.ApplyJonesTemplate(context, weights=weights, flags=flags, flag_value=32)
    fn = template.instantiate(queue, 300, 200, 58, 77)
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
    assert [name for name, _ in queue.launches] == ["ksp_apply_jones"]
    args = queue.launches[0][1]
    assert len(args) == 21

    def buf(name, present=True):
        return fn.buffer(name).buffer if present else None

    pointers = [buf("vis"), buf("weights", weights), buf("flags", flags), buf("jones"),
                buf("quad_antennas"), buf("quads"), buf("out_vis"), buf("out_weights", weights),
                buf("out_flags", flags)]  # fmt: skip
    for got, want in zip(args[:9], pointers):
        assert got is want
    for kind in kinds:
        assert (fn.buffer(kind) is fn.buffer("out_" + kind)) == in_place
    assert all(isinstance(a, np.int32) for a in args[9:])
    assert [int(a) for a in args[9:13]] == [300, 200, 58, 77]

    def stride(name, present=True):
        return fn.buffer(name).padded_shape[1] if present else 0

    strides = [stride("vis"), stride("weights", weights), stride("flags", flags), stride("jones"),
               stride("out_vis"), stride("out_weights", weights), stride("out_flags", flags)]  # fmt: skip
    assert [int(a) for a in args[13:20]] == strides
    if in_place:  # 500 rounded up to whole 128-byte rows
        want = [512, 512 if weights else 0, 512 if flags else 0, stride("jones")] * 2
        assert strides == want[:4] + want[:3]
    else:
        assert strides == [208, 224 if weights else 0, 256 if flags else 0, stride("jones"), 512,
                           224 if weights else 0, 256 if flags else 0]  # fmt: skip
    assert stride("jones") >= 58
    assert int(args[20]) == 32
    assert fn.buffer("jones").padded_shape[2] == 2
    assert fn.buffer("quad_antennas").padded_shape[1] == 2
    assert fn.buffer("quads").padded_shape[1] == 4


def test_between_solve_jones_and_compress(context, queue):
    """finalise -> solve_jones -> apply_jones -> compress: the averaged arrays are the inputs
    of both, each one buffer with one padded size, `jones` is one buffer, and `out_weights` is
    compress's `weights`."""
    channels, baselines, cf, n_inputs, n_quads = 4096, 200, 8, 16, 36
    rows = channels // cf
    finalise = device.FinaliseTemplate(context, channel_factor=cf).instantiate(
        queue, channels, baselines)  # fmt: skip
    solve = ingest.SolveJonesTemplate(context, corrections=True).instantiate(
        queue, rows, baselines, n_inputs)  # fmt: skip
    apply_jones = ingest.ApplyJonesTemplate(context).instantiate(
        queue, rows, baselines, n_inputs, n_quads)  # fmt: skip
    compress = ingest.CompressWeightsTemplate(context).instantiate(queue, rows, baselines)
    # more padding than any of them asks for, asked of one member of each compound
    accel.Dimension(baselines, min_padded_size=300).link(finalise.slots["weights"].dimensions[1])
    accel.Dimension(baselines, min_padded_size=700).link(compress.slots["weights"].dimensions[1])
    accel.Dimension(n_inputs, min_padded_size=40).link(solve.slots["jones"].dimensions[1])
    seq = accel.OperationSequence(
        queue, [("finalise", finalise), ("solve", solve), ("apply", apply_jones),
                ("compress", compress)],
        compounds={"vis": ["finalise:vis", "solve:vis", "apply:vis"],
                   "weights": ["finalise:weights", "solve:weights", "apply:weights"],
                   "flags": ["finalise:flags", "solve:flags", "apply:flags"],
                   "jones": ["solve:jones", "apply:jones"],
                   "cal_weights": ["apply:out_weights", "compress:weights"]})  # fmt: skip
    assert {"vis", "weights", "flags", "jones", "cal_weights", "apply:out_vis", "apply:out_flags",
            "apply:quad_antennas", "apply:quads", "compress:weights8"} <= set(seq.slots)  # fmt: skip
    seq()
    assert [name for name, _ in queue.launches] == [
        "ksp_average_finalise", "ksp_solve_jones", "ksp_apply_jones", "ksp_compress_weights"]  # fmt: skip
    final_args, solve_args, apply_args, compress_args = (launch[1] for launch in queue.launches)
    assert final_args[3] is solve_args[0] is apply_args[0] is seq.buffer("vis").buffer
    assert final_args[4] is solve_args[1] is apply_args[1] is seq.buffer("weights").buffer
    assert final_args[5] is solve_args[2] is apply_args[2] is seq.buffer("flags").buffer
    assert solve_args[5] is apply_args[3] is seq.buffer("jones").buffer
    assert apply_args[7] is compress_args[0] is seq.buffer("cal_weights").buffer
    assert apply_args[6] is seq.buffer("apply:out_vis").buffer
    assert len({id(a) for a in apply_args[:9]}) == 9  # out of place: nine buffers
    assert int(final_args[14]) == int(apply_args[14]) == seq.buffer("weights").padded_shape[1] == 320
    assert int(final_args[13]) == int(apply_args[13]) == seq.buffer("vis").padded_shape[1]
    assert int(final_args[15]) == int(apply_args[15]) == seq.buffer("flags").padded_shape[1]
    assert int(solve_args[16]) == int(apply_args[16]) == seq.buffer("jones").padded_shape[1] >= 40
    assert int(apply_args[18]) == int(compress_args[5]) == 704
    assert [int(a) for a in apply_args[9:13]] == [rows, baselines, n_inputs, n_quads]


def test_in_place_behind_finalise(context, queue):
    """Each pair in one compound with finalise's output: the matrices are applied in place."""
    finalise = device.FinaliseTemplate(context, channel_factor=4).instantiate(queue, 64, 40)
    apply_jones = ingest.ApplyJonesTemplate(context).instantiate(queue, 16, 40, 8, 10)
    kinds = ("vis", "weights", "flags")
    seq = accel.OperationSequence(
        queue, [("finalise", finalise), ("apply", apply_jones)],
        compounds={kind: ["finalise:" + kind, "apply:" + kind, "apply:out_" + kind]
                   for kind in kinds})  # fmt: skip
    seq()
    final_args, apply_args = (launch[1] for launch in queue.launches)
    for i, kind in enumerate(kinds):
        assert final_args[3 + i] is apply_args[i] is apply_args[6 + i] is seq.buffer(kind).buffer
        assert int(apply_args[13 + i]) == int(apply_args[17 + i]) == seq.buffer(kind).padded_shape[1]


# ------------------------------------------------------------------- the launcher's checks
@pytest.fixture(scope="module")
def lib():
    from katsdpsigproc_amd import _lib, build_native

    if not os.path.exists(_lib.LIB_PATH):
        build_native.build()
    return _lib.load()


ARRAYS = ["vis", "weights", "flags", "jones", "quad_antennas", "quads", "out_vis", "out_weights",
          "out_flags"]  # fmt: skip
STRIDES = ["vis", "weights", "flags", "jones", "out_vis", "out_weights", "out_flags"]


def test_argument_validation_without_gpu(lib):
    from katsdpsigproc_amd import _lib

    # never dereferenced: every call below fails its checks first. Nine arrays far apart.
    p = {name: ctypes.c_void_p((i + 1) << 32) for i, name in enumerate(ARRAYS)}

    def call(channels=4, baselines=8, n_inputs=4, n_quads=3, flag_value=128, **changed):
        a = dict(p, vis_stride=8, weights_stride=8, flags_stride=8, jones_stride=4,
                 out_vis_stride=8, out_weights_stride=8, out_flags_stride=8)  # fmt: skip
        a.update(changed)
        rc = lib.ksp_apply_jones(
            0, None, *(a[name] for name in ARRAYS), channels, baselines, n_inputs, n_quads,
            *(a[name + "_stride"] for name in STRIDES), flag_value)  # fmt: skip
        assert rc != 0
        return _lib.last_error()

    for name in ("vis", "jones", "quad_antennas", "quads", "out_vis"):
        assert f"invalid argument: {name} is NULL" in call(**{name: None})
    for name in ("weights", "out_weights"):
        assert "weights and out_weights must both be NULL or both be given" in call(**{name: None})
    for name in ("flags", "out_flags"):
        assert "flags and out_flags must both be NULL or both be given" in call(**{name: None})
    for bad in (0, -1):
        assert "invalid argument: channels must be at least 1" in call(channels=bad)
        assert "invalid argument: baselines must be at least 1" in call(baselines=bad)
        assert "invalid argument: n_quads must be at least 1" in call(n_quads=bad)
    for bad in (0, -2, 1, 3, 2047, 2049, 2050):
        assert "invalid argument: n_inputs must be even and 2..2048" in call(
            n_inputs=bad, jones_stride=4096)
    for bad in (0, 256, -128):
        assert "invalid argument: flag_value must be 1..255" in call(flag_value=bad)
    for name in ("vis", "weights", "flags", "out_vis", "out_weights", "out_flags"):
        assert f"invalid argument: {name}_stride is smaller than baselines" in call(
            **{name + "_stride": 7})
    assert "invalid argument: jones_stride is smaller than n_inputs" in call(jones_stride=3)
    assert "jones_stride is smaller" in call(n_inputs=2048, jones_stride=2047)
    # the order of the checks: everything wrong at once, then one thing less each time
    strides = {name + "_stride": -1 for name in STRIDES}
    wrong = dict(channels=0, baselines=0, n_inputs=0, n_quads=0, flag_value=0)
    assert "invalid argument: vis is NULL" in call(**wrong, **dict.fromkeys(p), **strides)
    assert "invalid argument: channels must" in call(**wrong, **strides)
    assert "invalid argument: baselines must" in call(**dict(wrong, channels=1), **strides)
    assert "invalid argument: n_inputs must" in call(**dict(wrong, channels=1, baselines=8), **strides)
    assert "invalid argument: n_quads must" in call(n_quads=0, flag_value=0, **strides)
    assert "invalid argument: flag_value must" in call(flag_value=0, **strides)
    assert "invalid argument: vis_stride is smaller than baselines" in call(**strides)
    assert "invalid argument: out_vis_stride is smaller than baselines" in call(
        **dict(strides, vis_stride=8))
    assert "invalid argument: jones_stride is smaller than n_inputs" in call(
        **dict(strides, vis_stride=8, out_vis_stride=8))  # fmt: skip
    assert "invalid argument: weights_stride is smaller than baselines" in call(
        **dict(strides, vis_stride=8, out_vis_stride=8, jones_stride=4))  # fmt: skip
    # an absent pair's strides are not looked at: the call gets as far as the next check
    none_w = dict(weights=None, out_weights=None, weights_stride=0, out_weights_stride=0)
    none_f = dict(flags=None, out_flags=None, flags_stride=0, out_flags_stride=0)
    assert "vis_stride is smaller" in call(**none_w, **none_f, vis_stride=7)

    # an output that overlaps its input without being it. The overlap checks are the last
    # before the launch, so a pair that passes is shown by the failure of a later pair.
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
        # in place, and arrays that only touch, pass this check: the flags' is reported
        if kind != "flags":
            for fine in (p[kind], at(kind, extent), at(kind, -extent)):
                assert "out_flags overlaps flags" in call(**{out: fine, "out_flags": at("flags", 1)})
    # a pair that is absent is not compared
    assert "out_flags overlaps flags" in call(**none_w, out_flags=at("flags", 1))


def test_header_binding_and_exports_agree(lib):
    from katsdpsigproc_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "katsdpsigproc_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declaration = re.search(r"int ksp_apply_jones\((.*?)\);", text, re.S)
    assert declaration is not None
    parameters = [" ".join(part.split()) for part in declaration.group(1).split(",")]
    argtypes = _lib.SIGNATURES["ksp_apply_jones"]
    assert len(parameters) == len(argtypes) == 23
    for parameter, argtype in zip(parameters, argtypes):
        assert ("*" in parameter) == (argtype is ctypes.c_void_p), parameter
        assert argtype in (ctypes.c_int, ctypes.c_void_p)
    names = [parameter.replace("*", " ").split()[-1] for parameter in parameters]
    assert names == ["device", "stream"] + ARRAYS + ["channels", "baselines", "n_inputs", "n_quads"] + [
        name + "_stride" for name in STRIDES] + ["flag_value"]  # fmt: skip
    assert hasattr(lib, "ksp_apply_jones") and "ksp_apply_jones" in _lib.declared_symbols()
    assert lib.ksp_abi_version() == _lib.ABI_VERSION == 5
    for name in ("ApplyJonesTemplate", "ApplyJones", "ApplyJonesHostFromDevice"):
        assert hasattr(ingest, name)
    assert hasattr(host, "ApplyJonesHost")
