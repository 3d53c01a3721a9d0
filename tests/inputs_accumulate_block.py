"""Dumps for the tests of ``rfi.ingest.AccumulateBlock``, shared by the tests with and without
a GPU, and what ``rfi.host.AveragerHost.add``, called dump by dump, makes of them.

A data set is MAX_DUMPS dumps of one shape with everything a test may ask for: weights, a
mask per channel and a mask per sample. A test takes the first D dumps and what its options
need. Data sets and host results are computed once per shape and options; they are shared, so
nobody writes to them.
"""

import functools

import numpy as np

MAX_DUMPS = 8


@functools.lru_cache(maxsize=None)
def make_dumps(channels, baselines, seed=0):
    """MAX_DUMPS of (vis, flags, weights, channel mask, full mask).

    Samples fall into classes by column (by position where there are fewer than 8 columns):
    never flagged (by flags or full mask), flagged in every dump, flagged in the first dump
    only, flagged in the last dump only, and flagged at random in about half the dumps; dump d
    flags with bit d. Weights are uniform in [0.5, 2] with some exact zeros. A few
    visibilities are around 2**-70 (their products with a flagged weight are denormal), a few
    are NaN or infinite, and a quarter are scaled by a power of two between 2**-20 and 2**20,
    a different one in every dump: float32 sums of such terms depend on their order."""
    rs = np.random.RandomState(1000003 * seed + 4099 * channels + baselines)
    shape = (channels, baselines)
    index = np.arange(baselines)[np.newaxis, :] + np.zeros(shape, int)
    if baselines < 8:
        index = np.arange(channels * baselines).reshape(shape)
    cls = index % 8
    dumps = []
    for d in range(MAX_DUMPS):
        vis = (rs.standard_normal(shape) + 1j * rs.standard_normal(shape)).astype(np.complex64)
        spread = rs.random_sample(shape) < 0.25
        vis[spread] *= (2.0 ** rs.randint(-20, 21, shape)).astype(np.float32)[spread]
        tiny = rs.random_sample(shape) < 0.05
        vis[tiny] *= np.float32(2.0**-70)
        special = rs.random_sample(shape)
        vis[special < 0.01] = np.nan
        vis[(special >= 0.01) & (special < 0.02)] = np.inf
        vis[(special >= 0.02) & (special < 0.03)] = complex(1.0, -np.inf)
        flagged = rs.random_sample(shape) < 0.5
        flagged[cls == 0] = False
        flagged[cls == 1] = True
        flagged[cls == 2] = d == 0
        flagged[cls == 3] = d == MAX_DUMPS - 1
        flags = np.where(flagged, np.uint8(1 << d), 0).astype(np.uint8)
        weights = rs.uniform(0.5, 2.0, shape).astype(np.float32)
        weights[rs.random_sample(shape) < 0.1] = 0
        channel_mask = np.where(rs.random_sample(channels) < 0.3, 0x08, 0).astype(np.uint8)
        full_mask = np.where(rs.random_sample(shape) < 0.3, 0x08, 0).astype(np.uint8)
        full_mask[cls == 0] = 0
        for a in (vis, flags, weights, channel_mask, full_mask):
            a.setflags(write=False)
        dumps.append((vis, flags, weights, channel_mask, full_mask))
    return tuple(dumps)


def select(dumps, use_weights=True, mode="NONE", same_channel_mask=True):
    """[(vis, flags, weights or None, mask or None)] of `dumps` for the options. An
    ``AccumulateBlock`` has one CHANNEL mask for all its dumps: `same_channel_mask` gives
    every dump that of the first."""
    out = []
    for vis, flags, weights, channel_mask, full_mask in dumps:
        if mode == "CHANNEL":
            mask = dumps[0][3] if same_channel_mask else channel_mask
        else:
            mask = full_mask if mode == "FULL" else None
        out.append((vis, flags, weights if use_weights else None, mask))
    return out


def host_accumulate(selected, mode="NONE", start=None):
    """(acc_vis, acc_weights, acc_flags) of ``AveragerHost`` after ``add`` on every dump of
    `selected` (from :func:`select`) in order, starting from the accumulators `start` (zero
    if None), which are left alone."""
    from katsdpsigproc_amd.rfi import host

    channels, baselines = selected[0][0].shape
    averager = host.AveragerHost(channels, baselines, 1, host.BackgroundFlags[mode])
    if start is not None:
        averager.acc_vis[...], averager.acc_weights[...], averager.acc_flags[...] = start
    for vis, flags, weights, mask in selected:
        averager.add(vis, flags, weights, mask)
    return averager.acc_vis, averager.acc_weights, averager.acc_flags


def same_bits(want, got):
    """Boolean array: equal bit patterns, or a NaN where the host has a NaN (its sign and
    payload are not arithmetic). complex64 is compared as pairs of float32."""
    assert want.dtype == got.dtype and want.shape == got.shape
    if want.dtype == np.uint8:
        return want == got
    want = np.ascontiguousarray(want).view(np.float32)
    got = np.ascontiguousarray(got).view(np.float32)
    return (want.view(np.uint32) == got.view(np.uint32)) | (np.isnan(want) & np.isnan(got))


def assert_same(want, got, what=""):
    ok = same_bits(want, got)
    if not ok.all():
        bad = ~ok
        w = np.ascontiguousarray(want).view(np.float32 if want.dtype != np.uint8 else np.uint8)
        g = np.ascontiguousarray(got).view(w.dtype)
        raise AssertionError(
            f"{what}: {np.count_nonzero(bad)} of {bad.size} differ, first at "
            f"{np.argwhere(bad)[0]}: want {w[bad][0]!r}, got {g[bad][0]!r}")  # fmt: skip
