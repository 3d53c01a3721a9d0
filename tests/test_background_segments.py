"""What the sweeps of tests/test_gpu_background_segments.py cover, stated from the launcher's
own segment geometry (ksp_background_median_filter_geometry), and the two CPU implementations
of the background filter against each other on the inputs those sweeps use. No GPU needed.

oracle.BackgroundMedianFilterHost is pinned to the reference's golden vectors at widths 5, 13
and from 33 on; rfi.host.BackgroundMedianFilterHost is a whole-array NumPy formulation that
shares no code with it. Their exact agreement at other widths is what makes the oracle a
reference for the GPU tests there.
"""

import ctypes
import os

import numpy as np
import pytest

from tests import inputs_background as ib


@pytest.fixture(scope="module")
def lib():
    from katsdpsigproc_amd import _lib, build_native

    if not os.path.exists(_lib.LIB_PATH):
        build_native.build()
    return _lib.load()


@pytest.fixture(scope="module")
def oracle():
    from oracle import rfi_oracle

    return rfi_oracle


# ------------------------------------------------------------------------------ the query
def test_geometry_is_the_documented_rule(lib):
    """seg_len = max(4 * width, ceil(channels / want_segs)) clamped to the band, want_segs =
    csplit, or enough for 8192 wavefronts when csplit is 0."""
    for width in (3, 13, 31):
        for channels in (1, 4 * width - 1, 4 * width, 4 * width + 1, 417, 4096, 12289):
            for baselines in (1, 64, 65, 8192):
                for csplit in (0, 1, 3, 4, 1000):
                    wave_cols = -(-baselines // 64)
                    want = csplit if csplit else -(-8192 // wave_cols)
                    seg_len = min(channels, max(4 * width, -(-channels // want)))
                    expected = (seg_len, -(-channels // seg_len))
                    assert ib.geometry(channels, baselines, width, csplit) == expected
    segs = ib.segments(417, *ib.geometry(417, 313, 13, 4))
    assert segs[0][0] == 0 and segs[-1][1] == 417
    assert all(a[1] == b[0] for a, b in zip(segs, segs[1:]))


def test_geometry_argument_checks(lib):
    from katsdpsigproc_amd import _lib

    seg_len, n_segs = ctypes.c_int(-7), ctypes.c_int(-7)
    out = (ctypes.byref(seg_len), ctypes.byref(n_segs))
    for width in (-1, 0, 1, 2, 4, 12, 32, 33, 63, 255):  # 33 .. 255: the wide-window kernel
        assert lib.ksp_background_median_filter_geometry(100, 10, width, 0, *out) != 0
        assert f"width {width}" in _lib.last_error()
        assert (seg_len.value, n_segs.value) == (-7, -7)
    assert lib.ksp_background_median_filter_geometry(100, 10, 13, -1, *out) != 0
    assert "csplit" in _lib.last_error()
    assert lib.ksp_background_median_filter_geometry(-1, 10, 13, 0, *out) != 0
    assert lib.ksp_background_median_filter_geometry(100, -1, 13, 0, *out) != 0
    assert lib.ksp_background_median_filter_geometry(100, 10, 13, 0, None, out[1]) != 0
    assert "NULL" in _lib.last_error()
    assert lib.ksp_background_median_filter_geometry(100, 10, 13, 0, out[0], None) != 0
    assert (seg_len.value, n_segs.value) == (-7, -7)
    # a band without samples launches nothing
    assert ib.geometry(0, 10, 13, 0) == (0, 0)
    assert ib.geometry(100, 0, 13, 4) == (0, 0)
    assert ib.geometry(0, 0, 3, 0) == (0, 0)


# ---------------------------------------------------------------------- what the sweeps run
def sweep_facts(width):
    half = width // 2
    residues, tails, before_last, multiples_of_4 = set(), set(), {}, 0
    for csplit, channels in ib.seam_sweep(width):
        seg_len, n_segs = ib.geometry(channels, ib.SWEEP_BASELINES, width, csplit)
        segs = ib.segments(channels, seg_len, n_segs)
        merges = [ib.segment_merges(channels, width, *seg) for seg in segs]
        assert not merges[0] and not merges[-1]  # the band's ends always take the sorted window
        if any(merges):
            residues.add(seg_len % width)
        tail = segs[-1][1] - segs[-1][0]
        tails.add(tail)
        if n_segs >= 3:
            before_last.setdefault(tail, set()).add(merges[-2])
            assert merges[-2] == (tail >= half)
        if csplit == 8:
            assert n_segs % 4 == 0 and sum(merges) >= n_segs - 3
            multiples_of_4 += 1
    return residues, tails, before_last, multiples_of_4


@pytest.mark.parametrize("width", ib.MERGE_WIDTHS)
def test_seam_sweep_covers_the_cases(width, lib):
    """The seam sweep does contain what it is meant to exercise. If this fails after a change
    to the sweep or to the launcher's geometry, the message says what is no longer run."""
    half = width // 2
    residues, tails, before_last, multiples_of_4 = sweep_facts(width)
    missing = set(range(width)) - residues
    assert not missing, f"no merging segment with seg_len mod {width} in {sorted(missing)}"
    missing = set(range(1, 2 * half + 3)) - tails
    assert not missing, f"no last segment of {sorted(missing)} channels"
    # the segment before the last merges when the last one holds at least `half` channels
    # (its halo then ends inside the band): both sides of that boundary, and every shorter
    # tail. (Width 3: a tail of half - 1 = 0 channels is no segment, so only one side exists.)
    assert before_last.get(half) == {True}, "tail of H channels: the segment before must merge"
    assert before_last.get(half + 1) == {True}
    for tail in range(1, half):
        assert before_last.get(tail) == {False}, f"tail of {tail} channels is not run"
    assert multiples_of_4 >= 3
    assert ib.seam_sweep_max_channels(width) == 32 * width + 24  # the launches stay tiny


@pytest.mark.parametrize("width", ib.MERGE_WIDTHS)
def test_fallback_sweep_geometry(width, lib):
    """Five segments, three of them merging, and a plant at every sample that each of them
    reads: its core, both halos, the first and the last sample."""
    channels, baselines, csplit = ib.fallback_shape(width)
    half = width // 2
    seg_len, n_segs = ib.geometry(channels, baselines, width, csplit)
    assert (seg_len, n_segs) == (4 * width + 3, 5)
    segs = ib.segments(channels, seg_len, n_segs)
    merges = [ib.segment_merges(channels, width, *seg) for seg in segs]
    assert merges == [False, True, True, True, False]
    rows, cols = ib.plant_positions(channels)
    assert len(set(cols // 64)) == channels == -(-baselines // 64)  # one plant per wave column
    assert cols.max() < baselines and np.array_equal(cols // 64, rows)
    for c_begin, c_end in segs[1:4]:
        assert set(range(c_begin - half, c_end + half)) <= set(rows.tolist())


@pytest.mark.parametrize("width", ib.ALL_WIDTHS)
def test_sorted_window_sweep_geometry(width, lib):
    """Three segments of 4 * width channels (and the tail that is left) for the long bands; one
    segment for a band shorter than a window."""
    long_bands, short_bands = ib.sorted_window_channels(width)
    half = width // 2
    for channels in long_bands:
        seg_len, n_segs = ib.geometry(channels, ib.SWEEP_BASELINES, width, 3)
        assert seg_len == 4 * width and n_segs == 2 + -(-(channels - 8 * width) // seg_len)
    tails = {channels - 8 * width for channels in long_bands}
    assert {1, half, half + 1, width - 1, width, width + 1, 2 * width, 4 * width} == tails
    for channels in short_bands:
        assert ib.geometry(channels, ib.SWEEP_BASELINES, width, 3) == (channels, 1)
    assert {1, 2, half, half + 1, width - 1, width, width + 1} == set(short_bands)


def test_inputs_cover_the_cases():
    """The generated bands do contain what the tests are meant to exercise."""
    tiny = np.finfo(np.float32).tiny
    for kind in ("cplx", "amp"):
        band = ib.make_band(105, ib.SWEEP_BASELINES, kind, seed=1)
        amp = np.abs(band).astype(np.float32) if kind == "cplx" else band
        assert band.dtype == (np.complex64 if kind == "cplx" else np.float32)
        assert np.isfinite(amp).all()  # or a whole wavefront would leave the merging median
        mag = np.abs(amp[:, 2 :: ib.N_FAMILIES])
        assert (mag == np.float32(2.0**-149)).any() and (mag >= np.float32(2.0**127)).any()
        assert ((mag > 0) & (mag < tiny)).sum() > 50
        alternating = mag[:, 1::2]
        assert (alternating[0::2] > 2.0**99).all() and (alternating[1::2] < 2.0**-98).all()
        ties = np.abs(amp[:, 1 :: ib.N_FAMILIES])
        assert set(np.unique(ties).tolist()) <= {0.0, 0.25, 0.375, 0.5, 0.75}
        assert (np.abs(amp[:, ib.CONSTANT_BASELINE]) == 0.375).all()
        assert (amp[:, ib.ZERO_BASELINE] == 0).all()
        assert (np.abs(amp[:, 0 :: ib.N_FAMILIES]) > 40).any()  # spikes
        if kind == "amp":
            assert (band < 0).any() and (np.signbit(band) & (band == 0)).any()
    chan, full = ib.make_masks(105, ib.SWEEP_BASELINES, 13, seed=2)
    assert 0.03 < np.count_nonzero(chan) / chan.size < 0.25
    assert 0.05 < np.count_nonzero(full) / full.size < 0.2
    assert full[2:17, 3:40].all() and full.max() > 1
    for kind in ("cplx", "amp"):
        planted = ib.scatter_plants(ib.make_band(105, 9, kind, seed=1), kind, seed=3)
        amp = np.abs(planted) if kind == "cplx" else planted
        assert np.isnan(amp).any() and (amp == np.inf).any()
        assert (amp == -np.inf).any() == (kind == "amp")


# ------------------------------------------------------- the oracle against the host class
def both_hosts(oracle, width, amplitudes, data, flags):
    from katsdpsigproc_amd.rfi import host

    with np.errstate(all="ignore"):
        a = oracle.BackgroundMedianFilterHost(width, amplitudes)(data, flags)
        b = host.BackgroundMedianFilterHost(width, amplitudes)(data, flags)
    assert a.dtype == b.dtype == np.float64 and not np.isnan(a).any()
    return a, b


@pytest.mark.parametrize("kind", ["cplx", "amp"])
@pytest.mark.parametrize("width", [7, 9, 11, 21, 31])
def test_oracle_agrees_with_host_class(width, kind, oracle):
    """Exact float64 agreement (the sign of a zero aside) of the two CPU implementations on the
    bands, masks and non-finite plants of the GPU sweeps: a band of three segments and a tail,
    and one that is a sample shorter than the window."""
    for channels, baselines in ((8 * width + width // 2, ib.SWEEP_BASELINES), (width - 1, 41)):
        band = ib.make_band(channels, baselines, kind, seed=width)
        chan, full = ib.make_masks(channels, baselines, width, seed=width + 1)
        planted = ib.scatter_plants(band, kind, seed=width + 2)
        for mode in ib.MODES:
            flags = ib.mode_flags(mode, chan, full, channels)
            for name, data in (("clean", band), ("planted", planted)):
                a, b = both_hosts(oracle, width, kind == "amp", data, flags)
                np.testing.assert_array_equal(
                    a, b, err_msg=f"{channels} x {baselines}, width {width}, {kind}, {mode}, {name}")
    # the single plants of the fallback sweep, on its first wave columns
    channels = ib.fallback_shape(width)[0]
    rows, cols = ib.plant_positions(channels)
    keep = cols < 64 * 3
    for value in ib.nonfinite_values(kind):
        data = ib.plant(ib.make_noise(channels, 64 * 3, kind, seed=width), rows[keep], cols[keep], value)
        a, b = both_hosts(oracle, width, kind == "amp", data, None)
        np.testing.assert_array_equal(a, b, err_msg=f"width {width}, {kind}, single {value}")
        assert np.isinf(a).any() == np.isinf(value)
