"""The NaN-deviation inputs of tests/inputs_nan_deviations.py, without a GPU: the expected
noise (``rfi.host.NoiseEstMADHost``) equals the reference's rule written out and the C oracle,
every class of column is what it claims to be, and no column with a NaN could pass under the
rule "a NaN is a non-zero value above +inf". The threshold inputs: every constructed window
fires in the control without its NaN, and no NaN sample is flagged by the host."""

import warnings

import numpy as np
import pytest

from katsdpsigproc_amd.rfi import host
from tests import inputs, inputs_nan_deviations as nd

# (tests/test_gpu_nan_deviations.py runs the kernels at the same lengths and width)
CHANNELS = nd.MAD_CHANNELS
COLUMNS = nd.MAD_COLUMNS


def expected_noise(dev):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # "no non-zero deviations"
        return host.NoiseEstMADHost()(dev).astype(np.float32)


def same(a, b):
    """Equal float32 arrays, NaN matching NaN of any payload."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype == np.float32 and a.shape == b.shape
    return (a == b) | (np.isnan(a) & np.isnan(b))


@pytest.fixture(scope="module")
def oracle():
    from oracle import rfi_oracle

    return rfi_oracle


@pytest.mark.parametrize("channels", CHANNELS)
def test_expected_noise(channels, oracle):
    dev = nd.nan_mad_case(channels, COLUMNS)
    want = expected_noise(dev)
    assert same(want, nd.reference_rule(dev)).all()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        assert same(want, oracle.NoiseEstMADHost()(dev).astype(np.float32)).all()
    # no case passes for nothing: with a NaN in the column and a finite expected value, the
    # rule that counts a NaN as a value above +inf gives another float32
    model = nd.kernel_rule_model(dev)
    has_nan = np.isnan(dev).any(axis=0)
    decided = has_nan & np.isfinite(want)
    assert not same(want[decided], model[decided]).any(), np.flatnonzero(decided)[
        same(want[decided], model[decided])]  # fmt: skip
    assert same(want[~has_nan], model[~has_nan]).all()  # (and the model is the rule without NaN)
    if channels >= 3:
        assert decided.sum() >= COLUMNS // 2


@pytest.mark.parametrize("channels", nd.GOLDEN_CHANNELS)
def test_reference_golden(channels):
    """The reference's own NoiseEstMADHost, recorded: the host class gives the same float64."""
    golden = np.load(nd.GOLDEN, allow_pickle=False)[f"mad_nan_{channels}"]
    dev = nd.nan_mad_case(channels, COLUMNS)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        np.testing.assert_array_equal(golden, host.NoiseEstMADHost()(dev))
    assert golden.dtype == np.float64 and np.isnan(golden).any() and np.isfinite(golden).any()


def counts(col):
    """(number of NaN, non-zero count without them, strictly below the upper median)."""
    a = np.abs(col)
    nz = np.sort(a[a > 0])
    below = int(np.count_nonzero(nz < nz[nz.size // 2])) if nz.size else 0
    return int(np.isnan(col).sum()), nz.size, below


@pytest.mark.parametrize("channels", CHANNELS)
def test_classes(channels):
    """Every class a length claims is present and is what its name says, by counts computed
    from the data."""
    dev = nd.nan_mad_case(channels, COLUMNS)
    names = nd.classes_at(channels)
    assert len(names) <= COLUMNS
    assert names == [name for name, least, _ in nd.CLASSES if least <= channels]
    if channels >= 10:
        assert len(names) == len(nd.CLASSES)
    if channels <= 3:  # the classes still possible at 1, 2 and 3 channels
        assert names == {
            1: ["control", "all"],
            2: ["control", "one_quiet"] + ["pattern_%08x" % p for p in nd.NAN_PATTERNS]
            + ["all_but_one", "all", "nan_and_zeros", "odd"],
            3: ["control", "one_quiet"] + ["pattern_%08x" % p for p in nd.NAN_PATTERNS]
            + ["majority", "all_but_one", "all", "nan_and_zeros", "even_first", "odd",
               "handovers"],
        }[channels]  # fmt: skip
    seen = set()
    for b in range(COLUMNS):
        name = nd.column_class(channels, b)
        seen.add(name)
        col = dev[:, b]
        bits = col.view(np.uint32)
        n_nan, n_nz, below = counts(col)
        n = channels
        if name == "control":
            assert n_nan == 0
        elif name == "one_quiet":
            assert n_nan == 1 and bits[np.isnan(col)][0] == 0x7FC00000
        elif name.startswith("pattern_"):
            assert n_nan == 1 and bits[np.isnan(col)][0] == int(name[8:], 16)
        elif name == "one_in_ten":
            assert n_nan == n // 10 and n_nz > n_nan
            where = np.flatnonzero(np.isnan(col))
            assert n < 100 or np.diff(where).max() > 1  # scattered, not one run
        elif name == "majority":
            assert n_nan > n // 2 and n_nan < n
        elif name == "all_but_one":
            assert n_nan == n - 1 and n_nz == 1 and col[~np.isnan(col)][0] == 2.0
        elif name == "all":
            assert n_nan == n
        elif name == "nan_and_zeros":
            assert n_nan >= 1 and n_nz == 0 and n_nan + np.count_nonzero(col == 0) == n
            assert n_nan < n
        elif name == "mixed":
            assert n_nan >= 1 and np.isposinf(col).any() and np.isneginf(col).any()
            assert (col == 0).any() and (bits == 0x80000000).any() and (bits == 0).any()
        elif name == "even_first":
            # even without the NaN, odd with them, and the upper median is the first sample
            # of its value: exactly rank = n_nz / 2 non-zero values lie below it
            assert n_nz % 2 == 0 and (n_nz + n_nan) % 2 == 1 and below == n_nz // 2
        elif name == "odd":
            assert n_nz % 2 == 1 and (n_nz + n_nan) % 2 == 0
        elif name == "even_tie":
            assert n_nz % 2 == 0 and (n_nz + n_nan) % 2 == 1 and below < n_nz // 2
        elif name == "handovers":
            pos = np.flatnonzero(np.isnan(col))
            want = {0, n - 1}
            for c in range(64, n, 64):
                want.update((c - 1, c))
            assert set(pos.tolist()) == want
            assert all(c - 1 in want and c in want for c in range(256, n, 256))
        else:
            raise AssertionError(name)
    assert seen == set(names)


# ------------------------------------------------------------------------------ thresholds
@pytest.mark.parametrize("channels", nd.THRESHOLD_CHANNELS)
def test_threshold_case(channels, oracle):
    dev, noise = nd.nan_threshold_case(channels)
    control, noise_c = nd.nan_threshold_case(channels, with_nan=False)
    isnan = np.isnan(dev)
    assert not np.isnan(control).any() and not np.isnan(noise).any()
    np.testing.assert_array_equal(noise, noise_c)
    np.testing.assert_array_equal(dev[~isnan], control[~isnan])
    assert not isnan[:, 0].any() and isnan[:, 6].all()
    assert isnan[[0, channels - 1], 7].all() and isnan[:, 7].sum() == 2
    assert isnan[:, 1].sum() == 5
    n_sigma = nd.THRESHOLD_N_SIGMA

    def flags(d, n_windows):
        out = host.ThresholdSumHost(n_sigma, n_windows)(d, noise)
        np.testing.assert_array_equal(out, oracle.ThresholdSumHost(n_sigma, n_windows)(d, noise))
        return out

    with_nan = {n: flags(dev, n) for n in range(1, 9)}
    without = {n: flags(control, n) for n in range(1, 9)}
    simple = host.ThresholdSimpleHost(n_sigma)(dev, noise)
    np.testing.assert_array_equal(simple, oracle.ThresholdSimpleHost(n_sigma)(dev, noise))
    for n in range(1, 9):
        assert not with_nan[n][isnan].any()  # a NaN sample is never flagged
    assert not simple[isnan].any()
    np.testing.assert_array_equal(simple, with_nan[1])
    assert not with_nan[8][:, 6].any()

    # the spikes fire alone, with their NaN neighbours or without
    for spike, nans in nd.THRESHOLD_SPIKES:
        assert isnan[list(nans), 2].all()
        assert without[1][spike, 2] and with_nan[1][spike, 2] and with_nan[8][spike, 2]
    assert with_nan[8][[1, channels - 2], 7].all()
    # each run fires in the control as a window of 2^k and as nothing narrower; with its NaN
    # it never fires
    for b, runs in nd.THRESHOLD_RUNS.items():
        for k, start in runs:
            run = slice(start, start + 2**k)
            assert isnan[run, b].sum() == 1 and isnan[start + 2**k // 2, b]
            assert not without[k][run, b].any(), (b, k)
            assert without[k + 1][run, b].all(), (b, k)
            assert not with_nan[8][run, b].any(), (b, k)
    # the hand-overs: both sides are NaN, and spikes around them fire
    for c in (8, 16, 32, 64, 128, 256):
        assert isnan[[c - 1, c], 8].all() and with_nan[1][c - 2, 8]
    for c in range(8, channels, 8):
        assert isnan[[c - 1, c], 9].all()
    assert with_nan[1][:, 9].sum() >= channels // 32 - 1
    pos = nd.chunk_positions(channels)
    assert isnan[:, 10].sum() == pos.size and isnan[pos, 10].all()
    if channels == 2100:
        # chunk 1's core, both halo ends and the shifted thread hand-overs, for every n_windows
        for n in range(1, 9):
            edge = nd.sum_edge(n)
            core = 2048 - 2 * edge
            for bound in (core, core - edge, core + edge, 8 - edge, core - edge + 8):
                if 1 <= bound < channels:
                    assert isnan[[bound - 1, bound], 10].all(), (n, bound)
        assert with_nan[1][:, 10].sum() > 20
        assert isnan[1200:, 11].sum() == (pos >= 1200).sum() > 0
        assert with_nan[1][1200:, 11][~isnan[1200:, 11]].all()
    else:
        assert pos.size == 0


def test_amplitude_case():
    """NaN in place of and next to the +-inf of columns 0-2 of nonfinite_amp_case; everything
    else, and nonfinite_amp_case itself, as it was."""
    amp, flags = inputs.nonfinite_amp_case()
    nan_amp, nan_flags = inputs.nonfinite_amp_nan_case()
    np.testing.assert_array_equal(flags, nan_flags)
    isnan = np.isnan(nan_amp)
    assert not np.isnan(amp).any()
    np.testing.assert_array_equal(amp[~isnan], nan_amp[~isnan])
    assert isnan[:, :3].any(axis=0).all() and not isnan[:, 3:].any()
    inf = np.isinf(amp)
    replaced = isnan & inf
    beside = isnan & ~inf & (np.roll(inf, 1, 0) | np.roll(inf, -1, 0))
    for col in range(3):
        assert replaced[:, col].any() and beside[:, col].any(), col
        assert np.isinf(nan_amp[:, col]).any(), col  # some infinities stay
    assert (replaced | beside)[isnan].all()
