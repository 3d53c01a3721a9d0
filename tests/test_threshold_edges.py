"""Inputs on the flagger's thresholds (``tests/inputs_threshold_edges.py``), on the CPU: the
premises of every case hold, the C oracle equals ``rfi.host`` on them in flags and noise -- the
GPU tests lean on the oracle -- and ``rfi.host`` equals the imported reference's own flags."""

import collections
import hashlib

import numpy as np
import pytest

from tests import inputs_threshold_edges as edges

ALL_NAMES = [name for path in edges.PATHS for name in edges.names(path)]


@pytest.fixture(scope="module")
def oracle():
    from oracle import rfi_oracle

    return rfi_oracle


@pytest.fixture(scope="module")
def golden():
    return np.load(edges.GOLDEN, allow_pickle=False)


@pytest.mark.parametrize("path", list(edges.PATHS))
def test_names(path):
    """The names the tests are parametrised with are the cases there are."""
    assert [case.name for case in edges.cases(path)] == edges.names(path)


@pytest.mark.parametrize("name", ALL_NAMES)
def test_premises(name):
    case = edges.by_name(name)
    assert edges.check_premises(case) == len(case.planted) >= case.vis.shape[1]
    assert case.vis.dtype == (np.float32 if case.amplitudes else np.complex64)
    if not case.amplitudes:
        assert not case.vis.imag.any()


@pytest.mark.parametrize("path", list(edges.PATHS))
def test_coverage(path):
    """Every (window, direction) that exists, a replaced window and both directions of the simple
    threshold, at every shape of the path; and where the windows lie."""
    shapes, windows = edges.PATHS[path]
    for shape in shapes:
        mine = [c for c in edges.cases(path) if c.vis.shape == shape]
        got = collections.Counter((c.kind, c.window, c.direction, c.replaced) for c in mine)
        want = {("sum", w, d, False) for w in windows for d in edges.DIRECTIONS[w]}
        want |= {("simple", 1, "exact", False), ("simple", 1, "float32", False)}
        assert want <= set(got)
        assert any(c.replaced for c in mine)
        assert ("sum", 1, "float32", False) not in got  # (it cannot exist: the module says why)
        for case in mine:
            w, firsts = case.window, {c for _, c, _ in case.planted}
            if len(edges._roles(w, case.direction, case.replaced)[0]) < 4:
                assert 0 in firsts and shape[0] - w in firsts
            if w > 1:
                # across a lane boundary, by every number of channels (three beyond 8)
                before = {lane - c for c in firsts for lane in range(64, shape[0], 64)
                          if c < lane < c + w}
                assert before >= set(edges._straddles(w)), case.name
                if path == "long":
                    for boundary in (4096, 8192):
                        if boundary < shape[0]:
                            assert {boundary - c for c in firsts if c < boundary < c + w} \
                                >= set(edges._boundary_straddles(w)), case.name
    if path == "fused4":
        mine = edges.cases(path)
        for field, values in (("width", {13, 31}), ("amplitudes", {False, True}),
                              ("keep_deviations", {False, True})):  # fmt: skip
            assert {getattr(c, field) for c in mine} == values
        assert {c.n_windows for c in mine if c.kind == "sum"} >= {4, 5, 6, 8}
        assert any(c.in_flags is not None for c in mine)


@pytest.mark.parametrize("name", ALL_NAMES)
def test_oracle_equals_host(name, oracle):
    case = edges.by_name(name)
    _, noise, flags, _ = case.host_stages()
    ref_flags, ref_noise = oracle.flagger_full(
        case.vis, case.in_flags, width=case.width, amplitudes=case.amplitudes, threshold=case.kind,
        n_sigma=case.n_sigma, n_windows=case.n_windows, threshold_falloff=case.threshold_falloff)  # fmt: skip
    np.testing.assert_array_equal(noise, ref_noise)
    np.testing.assert_array_equal(flags, ref_flags)


@pytest.mark.parametrize(
    "name", [n for n in ALL_NAMES if edges.by_name(n).vis.shape[0] <= edges.GOLDEN_MAX_CHANNELS])
def test_host_equals_reference(name, golden):
    """``rfi.host`` against the flags the reference itself gave."""
    case = edges.by_name(name)
    flags = np.ascontiguousarray(case.host_stages()[2], np.uint8)
    assert int(np.count_nonzero(flags)) == int(golden[name + "_count"])
    assert hashlib.sha256(flags.tobytes()).hexdigest() == str(golden[name + "_sha"])
    if case.vis.shape[0] <= edges.GOLDEN_PACKED_CHANNELS:
        stored = np.unpackbits(golden[name + "_flags"])[: flags.size].reshape(flags.shape)
        np.testing.assert_array_equal(stored, flags)


@pytest.mark.parametrize("args", edges.BAND_END, ids=lambda a: f"{a[0]}_{a[1][0]}x{a[1][1]}_w{a[2]}")
def test_band_end(args, oracle):
    """The premises of ``band_end_case`` are asserted where it is built; the oracle flags nothing
    either, with the host's noise."""
    case = edges.band_end_case(*args)
    ref_flags, ref_noise = oracle.flagger_full(
        case.vis, width=case.width, n_sigma=case.n_sigma, n_windows=case.n_windows,
        threshold_falloff=case.threshold_falloff)  # fmt: skip
    np.testing.assert_array_equal(case.host_stages()[1], ref_noise)
    assert not ref_flags.any()


def test_float32_deviations_decide_wrongly():
    """What the cases are for, stated once without the generator's help: at every planted window
    the flags from float32 deviations are wrong."""
    for case in edges.all_cases():
        dev, noise, exact, rounded = case.host_stages()
        for b, c, w in case.planted:
            assert not np.array_equal(exact[c : c + w, b], rounded[c : c + w, b]), case.name
