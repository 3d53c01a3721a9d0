"""Inputs for what a workgroup of the persistent ring kernel (csrc/ring_kernel.h) carries from
one strip of 8 baselines to its next, and a CPU model of the decision that uses it.

Wavefront ``w`` of a workgroup owns baseline ``8 * strip + w`` of every strip the workgroup
takes, and hands the top 8 bits of that baseline's MAD key bin to the search of the next
(``mad_hint`` of the strip loop, ``top_hint`` of ``mad_noise`` in csrc/fused_common.h). Which
strip follows which is decided by a race for tickets, so every family here assigns its kinds of
baseline in random order, separately for each of the 8 positions ``b % 8``: whatever the order
of the strips, neighbouring strips differ.

:func:`mad_bin` classifies the oracle's float64 deviations the way ``mad_noise`` does and
:func:`hinted_search` is a model of its hinted search with the true hit test or a wrong one;
tests/test_ring_strips.py uses them to show, without a GPU, that each family reaches what it is
for. Importing this module touches neither the GPU nor the oracle.

All families: 4096 channels, complex64, ``8 * (2 * n_cu + 1)`` baselines -- two strips per
workgroup and one over, so every workgroup runs a second strip."""

import collections
import functools

import numpy as np

from tests import inputs

CHANNELS = 4096
WIDTH = 13
STRIP = 8  # baselines per strip: one per wavefront
DEFAULT_CU = 256
TOTAL = CHANNELS  # samples the MAD ranks

Family = collections.namedtuple("Family", "name vis kind kinds extra")
Family.__doc__ = """``vis`` [channels][baselines]; ``kind[b]`` indexes ``kinds`` (names);
``extra``: what only one family has."""


def compute_units(context):
    """The device's compute-unit count as the launcher sees it, 256 if it is not told."""
    return getattr(context.device, "compute_units", None) or DEFAULT_CU


def baselines_for(n_cu=DEFAULT_CU):
    return STRIP * (2 * n_cu + 1)


# --------------------------------------------------------------------------- the classifier
def keys_of(dev64):
    """The kernel's 15-bit keys: the top 16 bits of the pattern of ``float32(|dev|)``, rounded
    up, so that key 0 means a float32 zero."""
    with np.errstate(over="ignore", invalid="ignore"):
        d32 = np.abs(dev64).astype(np.float32)
    pattern = d32.view(np.uint32).astype(np.int64) & 0x7FFFFFFF
    return ((pattern + 0xFFFF) >> 16).astype(np.uint16)


class SortedKeys:
    """The sorted keys of many baselines, for counting: ``less(b, t)`` = how many keys of
    baseline ``b`` lie below ``t``, for arrays of ``b`` and ``t``."""

    def __init__(self, keys):
        keys = np.asarray(keys)
        if keys.ndim == 1:
            keys = keys[:, np.newaxis]
        self.channels, self.baselines = keys.shape
        self.sorted = np.sort(keys, axis=0)
        offset = np.arange(self.baselines, dtype=np.uint32) << 16
        self.flat = (self.sorted.T.astype(np.uint32) + offset[:, np.newaxis]).ravel()

    def less(self, baseline, t):
        baseline = np.asarray(baseline, np.int64)
        query = (baseline << 16) + np.asarray(t, np.int64)
        return np.searchsorted(self.flat, query.astype(np.uint32)) - baseline * self.channels

    def at(self, baseline, rank):
        return self.sorted[rank, baseline].astype(np.int64)


MadBin = collections.namedtuple("MadBin", "keys zeros tiny rank searched key top lb cnt")
MadBin.__doc__ = """Per baseline, what ``mad_noise`` decides. ``keys``: :class:`SortedKeys`;
``zeros``: deviations that are zero; ``tiny``: deviations of +-2^-150, zero as float32 but not
zero; ``rank = (total + zeros) // 2``; ``searched``: False where the kernel returns before the
search and leaves the hint as it found it (every deviation zero, or the median among the
+-2^-150); ``key``: the key at that rank and ``top = key >> 7`` (-1 where not searched); for
the hint given, ``lb``: keys whose top is below it, ``cnt``: keys whose top equals it."""


def mad_bin(dev64, hint=None):
    """Classify float64 deviations [channels][baselines]. `hint`: a top (scalar, or one per
    baseline) for ``lb`` and ``cnt``, which are None without it."""
    total = dev64.shape[0]
    keys = SortedKeys(keys_of(dev64))
    zeros = np.count_nonzero(dev64 == 0, axis=0).astype(np.int64)
    tiny = np.count_nonzero(np.abs(dev64) == 2.0 ** -150, axis=0).astype(np.int64)
    zero_keys = np.count_nonzero(keys.sorted == 0, axis=0)
    assert np.array_equal(zero_keys, zeros + tiny)  # nothing else is zero as float32
    rank = (total + zeros) // 2
    searched = (zeros != total) & (rank >= zero_keys)
    every = np.arange(dev64.shape[1])
    key = np.where(searched, keys.at(every, np.minimum(rank, total - 1)), -1)
    top = np.where(searched, key >> 7, -1)
    lb = cnt = None
    if hint is not None:
        h = np.broadcast_to(np.asarray(hint, np.int64), every.shape)
        lb = keys.less(every, h << 7)
        cnt = keys.less(every, (h + 1) << 7) - lb
    return MadBin(keys, zeros, tiny, rank, searched, key, top, lb, cnt)


def narrowed_lower_below(dev64, cap):
    """Per baseline of float64 deviations: the key bin of the MAD's rank holds more than `cap`
    samples (``mad_noise`` then narrows it to the one float32 value at the rank), at most `cap`
    share that value, the count of non-zero deviations is even, the upper median is the first
    sample of that value, and the lower median, the largest value below it, has the same key:
    it lies below the narrowed bin but not below the key's."""
    total = dev64.shape[0]
    with np.errstate(over="ignore", invalid="ignore"):
        pattern = np.abs(dev64).astype(np.float32).view(np.uint32).astype(np.int64)
    pattern = np.sort(pattern, axis=0)
    key = (pattern + 0xFFFF) >> 16
    zeros = np.count_nonzero(dev64 == 0, axis=0)
    out = np.zeros(dev64.shape[1], bool)
    for b in np.flatnonzero(zeros != total):
        rank = (total + zeros[b]) // 2
        p, k = pattern[:, b], key[:, b]
        if rank < np.count_nonzero(k == 0) or np.count_nonzero(k == k[rank]) <= cap:
            continue
        first = np.searchsorted(p, p[rank])
        out[b] = (np.count_nonzero(p == p[rank]) <= cap and (total + zeros[b]) % 2 == 0
                  and rank == first and k[rank - 1] == k[rank])
    return out


TRUE, LE_UPPER, LT_LOWER, ALWAYS = "true", "rank <= lb + cnt", "lb < rank", "always hit"
LE_LOWER = "lb <= rank + 1"  # the lower test too lax by one, as LE_UPPER is the upper one
WRONG_VARIANTS = (LE_UPPER, LT_LOWER, ALWAYS, LE_LOWER)


def hinted_search(keys, rank, hint, variant=TRUE, baseline=None):
    """Model of the hinted bin search of ``mad_noise``: follow the hinted top bits down the bit
    planes and count the keys below them (``lb``) and under them (``cnt``); on a hit take the
    top bits from the hint and decide the 7 low bits one at a time, otherwise decide all 15.
    A step sets a bit if the keys below the bin that it would then start number at most `rank`;
    on either path the count carried along equals the number of keys below the prefix decided
    so far (``lb`` is that number for the hinted prefix), so a step counts the keys below its
    candidate prefix.

    `keys`: a :class:`SortedKeys`, or the keys of one baseline; `rank`, `hint` (negative: none)
    and `baseline` (default: every one in turn) are arrays over the queries. `variant`: the hit
    test, the true one or a wrong one. Returns (key bin, one-bit steps taken) per query."""
    if not isinstance(keys, SortedKeys):
        keys = SortedKeys(keys)
    if baseline is None:
        baseline = np.arange(keys.baselines)
    baseline = np.asarray(baseline, np.int64)
    rank = np.broadcast_to(np.asarray(rank, np.int64), baseline.shape)
    hint = np.broadcast_to(np.asarray(hint, np.int64), baseline.shape)
    h = np.maximum(hint, 0)
    lb = keys.less(baseline, h << 7)
    cnt = keys.less(baseline, (h + 1) << 7) - lb
    hit = {
        TRUE: (lb <= rank) & (rank < lb + cnt),
        LE_UPPER: (lb <= rank) & (rank <= lb + cnt),
        LT_LOWER: (lb < rank) & (rank < lb + cnt),
        ALWAYS: np.ones(baseline.shape, bool),
        LE_LOWER: (lb <= rank + 1) & (rank < lb + cnt),
    }[variant] & (hint >= 0)
    K = np.where(hit, h << 7, 0)
    miss = np.flatnonzero(~hit)
    for bit in range(14, -1, -1):
        who = miss if bit >= 7 else slice(None)
        test = K[who] | (1 << bit)
        take = keys.less(baseline[who], test) <= rank[who]
        K[who] = np.where(take, test, K[who])
    return K, np.where(hit, 7, 15)


# --------------------------------------------------------------------------------- builders
@functools.lru_cache(maxsize=2)
def noise_block(baselines):
    """``generate_data`` noise, seed 5, shared by the families and read-only."""
    vis = inputs.generate_data(CHANNELS, baselines, seed=5)
    vis.setflags(write=False)
    return vis


def scaled(vis, factor):
    """Multiplied in complex128, rounded once."""
    return (vis.astype(np.complex128) * factor).astype(np.complex64)


def shuffled_kinds(rs, baselines, shares):
    """A kind for every baseline: at each position ``b % 8`` the kinds in the proportions
    `shares` (to the nearest baseline, the first kind takes up the difference), in random order."""
    kind = np.empty(baselines, np.int64)
    shares = np.asarray(shares, np.float64) / np.sum(shares)
    for w in range(STRIP):
        n = len(range(w, baselines, STRIP))
        count = np.floor(shares * n).astype(np.int64)
        count[0] += n - count.sum()
        kind[w::STRIP] = rs.permutation(np.repeat(np.arange(len(shares)), count))
    return kind


def position_counts(kind, n_kinds):
    """[8][n_kinds]: how many baselines of each kind at each position ``b % 8``."""
    return np.array([np.bincount(kind[w::STRIP], minlength=n_kinds) for w in range(STRIP)])


def binades(baselines=baselines_for()):
    """Baseline b scaled by 2^e[b], e uniform in -60 .. 60: amplitudes on both sides of the
    short-division limits 2^-63 and 2^65 of ``ksp_abs_range_key``, and a hint that almost never
    fits the next baseline."""
    e = np.random.RandomState(1).randint(-60, 61, baselines)
    vis = scaled(noise_block(baselines), 2.0 ** e[np.newaxis, :])
    return Family("binades", vis, e + 60, tuple(f"2^{k}" for k in range(-60, 61)), {"e": e})


# Noise of unit variance per component has a MAD of about 0.45 after the median filter, next to
# the limit of a bin at 0.5; times 1.5 it lies in the middle of the bin of 2^-1.
NEIGHBOUR_BASE = 1.5
NEIGHBOUR_TOP = 126  # the biased exponent of 2^-1: the top of that bin


def neighbours(baselines=baselines_for()):
    """The same noise scaled by 1.5 times 1/2, 1 or 2, a third each: the bin's top is
    ``NEIGHBOUR_TOP`` - 1, + 0 or + 1, and a hint is wrong by exactly one either way."""
    kind = shuffled_kinds(np.random.RandomState(2), baselines, [1, 1, 1])
    vis = scaled(noise_block(baselines), NEIGHBOUR_BASE * 2.0 ** (kind - 1)[np.newaxis, :])
    return Family("neighbours", vis, kind, ("A-1", "A", "A+1"), {})


# ---- edges. Deviations are x = +-k * 2^-23 for integers k; the bin of top EDGE_TOP (keys
# 0x3a80 .. 0x3aff: float32 patterns 0x3a7f0001 .. 0x3aff0000) holds K_IN_LO <= k <= K_IN_HI.
EDGE_TOP = 117  # the biased exponent of 2^-10
K_LO, K_IN_LO, K_IN_HI, K_HI = 1024, 8161, 16320, 65536
# k = 8161 .. 8191 and 16321 .. 16383 have the 7 top mantissa bits set and low bits that are not
# zero: the key's rounding carries them into the next top (8160 and 16320 are the last it does not)
K_CARRY = 31, 63
K_FLAGGED = 1 << 20  # 2^-3: far above 11 sigma of a MAD near 2^-10
EDGE_SLOTS = CHANNELS // 8  # excursions sit at channels 8 k + 4: at most 2 in any window of 13
EDGE_CLASSES = ("last_of_h", "first_above", "first_of_h", "last_below")
# class -> (rank - lb, rank - (lb + cnt)); None: not fixed by the class
EDGE_RIMS = {"last_of_h": (None, -1), "first_above": (None, 0), "first_of_h": (0, None),
             "last_below": (-1, None), "straddle": (0, None)}  # fmt: skip
EDGE_KINDS = tuple(f"filler_h{s:+d}" if s else "filler_h" for s in (-1, 0, 1)) + tuple(
    f"{cls}_{parity}" for cls in EDGE_CLASSES for parity in ("even", "odd")) + ("straddle_even",)  # fmt: skip


def _edge_baseline(rs, name):
    """The 512 excursions x (float64; 0: none) of one constructed baseline, in slot order."""
    cls, parity = name.rsplit("_", 1)
    n = EDGE_SLOTS - (parity == "odd")  # non-zero deviations
    m = n // 2  # rank among the non-zero ones: the (upper) median
    n_in = int(rs.randint(1, 150))  # on both sides of the 64 that are ranked one per lane
    if cls == "last_of_h":
        n_below = m + 1 - n_in
    elif cls == "first_above":
        n_below = m - n_in
    elif cls == "last_below":
        n_below = m + 1
    else:  # first_of_h, straddle
        n_below = m
    n_above = n - n_below - n_in
    assert n_below >= 1 and n_in >= 1 and n_above >= 4
    below = np.sort(rs.randint(K_LO, K_IN_LO, n_below))
    inside = np.sort(np.where(rs.random_sample(n_in) < 0.2, K_IN_LO + rs.randint(0, K_CARRY[0], n_in),
                              rs.randint(K_IN_LO, K_IN_HI + 1, n_in)))  # fmt: skip
    above = np.sort(np.where(rs.random_sample(n_above) < 0.2, K_IN_HI + 1 + rs.randint(0, K_CARRY[1], n_above),
                             rs.randint(K_IN_HI + 1, K_HI + 1, n_above)))  # fmt: skip
    above[-3:] = K_FLAGGED
    # every other time the samples on the rim are the very last and first values of their tops
    if cls == "straddle" or rs.randint(2):
        below[-1] = K_IN_LO - 1
        inside[0] = K_IN_LO
        inside[-1] = max(inside[-1], K_IN_HI if n_in > 1 else K_IN_LO)
        above[0] = K_IN_HI + 1
    k = np.concatenate([below, inside, above]).astype(np.float64)
    x = np.zeros(EDGE_SLOTS)
    x[rs.permutation(EDGE_SLOTS)[:n]] = k * 2.0 ** -23 * rs.choice([-1.0, 1.0], n)
    return x


def edges(baselines=baselines_for()):
    """Constructed baselines whose MAD rank lies on the rim of the bin of top ``EDGE_TOP``: a
    real level of 1 with excursions 1 + x at channels 8 k + 4, so every median is 1 and the
    deviations are x exactly; 512 (even) or 511 (odd) of them. Among fillers of noise whose top
    is ``EDGE_TOP`` - 1, + 0 or + 1, so that the hints that meet them are those three.
    ``extra["x"]``: [512][baselines], the excursion of slot k (0 for none and in the fillers)."""
    rs = np.random.RandomState(3)
    n_cls = len(EDGE_KINDS) - 3
    kind = shuffled_kinds(rs, baselines, [0.18] * 3 + [0.46 / n_cls] * n_cls)
    shift = EDGE_TOP - NEIGHBOUR_TOP + np.where(kind < 3, kind - 1, 0)
    vis = scaled(noise_block(baselines), NEIGHBOUR_BASE * 2.0 ** shift[np.newaxis, :])
    x = np.zeros((EDGE_SLOTS, baselines))
    for b in np.flatnonzero(kind >= 3):
        x[:, b] = _edge_baseline(rs, EDGE_KINDS[kind[b]])
        vis[:, b] = 1.0
        vis[4::8, b] = (1.0 + x[:, b]).astype(np.float32)
    return Family("edges", vis, kind, EDGE_KINDS, {"x": x})


# ---- mixed
MIXED_KINDS = ("noise", "zero", "constant", "quantised", "tiny", "nan", "inf", "overflow",
               "2^-140", "2^100")  # fmt: skip
# Amplitudes in units of 2^-149 at a band edge, on a level of 20: windows with an even number of
# samples give deviations of +-2^-150 there, (how many of them, how many other non-zero ones) --
# found by search, like ``inputs.denormal_case``. A baseline with such edges and nothing else has
# its median among the +-2^-150.
TINY_EDGES = [([21] * 6, (1, 0)), ([19] * 6, (1, 0)), ([18] * 5 + [19], (2, 1)),
              ([18, 18, 18, 18, 21, 19, 20, 20, 18], (3, 2))]  # fmt: skip


def _tiny_baseline(rs):
    units = np.full(CHANNELS, 20.0)
    ends = [rs.randint(len(TINY_EDGES)) if use else None for use in ((1, 0), (0, 1), (1, 1))[rs.randint(3)]]
    if ends[0] is not None:
        edge = TINY_EDGES[ends[0]][0]
        units[: len(edge)] = edge
    if ends[1] is not None:
        edge = TINY_EDGES[ends[1]][0]
        units[CHANNELS - len(edge) :] = edge[::-1]
    return (units * 2.0 ** -149).astype(np.float32)


def mixed(baselines=baselines_for()):
    """Ordinary noise interleaved with baselines that leave the streaming path or the search:
    all zero and constant (no deviation: NaN noise, no search), quantised (as in
    ``test_degenerate_full_band``), a majority of +-2^-150 among the non-zero deviations (the
    median is one of them, no search), one NaN or one infinity (the sorted-window median),
    a run of 20 samples whose amplitude overflows, noise scaled by 2^-140 (subnormal) and by
    2^100. Every kind occurs among the first and among the last 16 baselines."""
    rs = np.random.RandomState(4)
    n_kinds = len(MIXED_KINDS)
    kind = shuffled_kinds(rs, baselines, [0.37] + [0.07] * (n_kinds - 1))
    for part in (slice(0, 16), slice(baselines - 16, baselines)):
        kind[part] = rs.permutation(np.concatenate([np.arange(n_kinds), rs.randint(0, n_kinds, 16 - n_kinds)]))
    vis = np.array(noise_block(baselines))
    channel = np.arange(CHANNELS)
    for b in np.flatnonzero(kind):
        name = MIXED_KINDS[kind[b]]
        if name == "zero":
            vis[:, b] = 0
        elif name == "constant":
            vis[:, b] = 3 + 4j
        elif name == "quantised":
            which = rs.randint(4)
            if which == 0:
                vis[:, b] = rs.randint(0, 4, CHANNELS)
            elif which == 1:
                vis[:, b] = rs.randint(0, 50, CHANNELS) * 0.25
                vis[100, b] = 1000.0
            elif which == 2:
                vis[:, b] = rs.randint(0, 1000, CHANNELS) * 2.0 ** -10
            else:
                vis[:, b] = channel % 7 + 1j * (channel % 5)
        elif name == "tiny":
            vis[:, b] = _tiny_baseline(rs)
        elif name == "nan":
            vis[rs.choice([0, 3, 64, 4095, rs.randint(CHANNELS)]), b] = [np.nan, np.nan + 1j][rs.randint(2)]
        elif name == "inf":
            vis[rs.choice([0, 63, 4092, 4095, rs.randint(CHANNELS)]), b] = [np.inf, np.inf * 1j][rs.randint(2)]
        elif name == "overflow":
            start = rs.randint(0, CHANNELS - 20)
            vis[start : start + 20, b] = 3e38 + 3e38j
        elif name == "2^-140":
            vis[:, b] = scaled(vis[:, b], 2.0 ** -140)
        elif name == "2^100":
            vis[:, b] = scaled(vis[:, b], 2.0 ** 100)
    return Family("mixed", vis, kind, MIXED_KINDS, {})


FAMILIES = {"binades": binades, "neighbours": neighbours, "edges": edges, "mixed": mixed}
