"""The flagger's options, pairwise: a table of cases over every option of the flagger, the
inputs of each case and its expected results.

``tests/test_gpu_flagger.py`` varies one option at a time around the benchmark's values. Here
every pair of levels of every two factors of :data:`FACTORS` occurs in at least one case of
:data:`CASES` (``tests/test_flagger_matrix.py`` proves it), so that a kernel or a piece of
wiring that is right for every option alone and wrong for one combination has a case that
meets it. The table is a literal list: the same on every run and every machine.

Three blocks make up :data:`CASES`:

* :data:`PAIRWISE`, a greedy pairwise cover of the factors (none of its cases is eligible for
  the persistent ring kernel);
* :data:`FUSED_CLASSES`, hand-placed cases under ``engine="auto"``. A pairwise cover leaves
  four cases in five to the forced sequence and most of the others to widths or sizes the
  fused kernels decline, so on its own it would run some fused kernels once or never. These
  cases run every kernel class of the fused dispatch (4, 16 and 64 channels per lane, long
  bands in strips of 4 and of 3 baselines) at least twice, and each of them with amplitude
  input, a mask, kept deviations, the simple threshold, the other flag value and padded
  rows at least once;
* :data:`RING`, hand-placed cases that satisfy the seven-way conjunction the ring kernel
  needs, which a pairwise cover does not produce.

Importing this module touches neither a GPU nor the oracle; the inputs and references are
built on demand and cached, so the CPU and the GPU tests of one process share them.
"""

import functools
import itertools
from collections import namedtuple

import numpy as np

from tests import inputs

FACTORS = (
    ("channels", (40, 200, 700, 3000, 4096, 5000, 9100, 13000)),
    ("width", (3, 7, 13, 21, 31, 63)),
    ("threshold", ("simple", "sum1", "sum4", "sum6", "sum8")),
    ("mask", ("NONE", "CHANNEL", "FULL")),
    ("input", ("complex", "amplitude")),
    ("keep_deviations", (False, True)),
    ("baselines", (3, 8, 11, 17)),
    ("flag_value", (1, 0x80)),
    ("sigma", ((11.0, 1.2), (6.0, 1.5))),  # (n_sigma, threshold_falloff)
    ("engine", ("auto", "seq_mad_cm", "seq_madt_cm", "seq_mad_t", "seq_madt_t")),
    ("data", ("sparse", "broad", "ties", "specials")),
    ("vis_pad", (0, 16)),
)
FACTOR_NAMES = tuple(name for name, _ in FACTORS)

_Case = namedtuple("_Case", FACTOR_NAMES + ("seed",))


class Case(_Case):
    """One row of the table: a level of every factor and the seed of its data."""

    __slots__ = ()

    @property
    def n_sigma(self):
        return self.sigma[0]

    @property
    def threshold_falloff(self):
        return self.sigma[1]

    @property
    def sum_threshold(self):
        return self.threshold != "simple"

    @property
    def n_windows(self):
        """Windows of SumThreshold; 1 for the simple threshold (as the fused kernels count)."""
        return int(self.threshold[3:]) if self.sum_threshold else 1

    @property
    def amplitudes(self):
        return self.input == "amplitude"

    @property
    def forced_sequence(self):
        return self.engine != "auto"

    @property
    def noise_transposed(self):
        """NoiseEstMADT (baseline-major) or NoiseEstMAD; ``auto`` takes the benchmark's."""
        return self.engine in ("auto", "seq_madt_cm", "seq_madt_t")

    @property
    def threshold_transposed(self):
        return self.engine in ("auto", "seq_mad_t", "seq_madt_t")

    @property
    def id(self):
        return "c{}-w{}-{}-{}-{}-{}-b{}-fv{}-s{:g}-{}-{}-p{}".format(
            self.channels, self.width, self.threshold, self.mask.lower(),
            "amp" if self.amplitudes else "cplx", "dev" if self.keep_deviations else "nodev",
            self.baselines, self.flag_value, self.n_sigma, self.engine, self.data, self.vis_pad)


# fmt: off
PAIRWISE = (
    (5000, 63, "simple", "NONE", "complex", False, 3, 128, (6.0, 1.5), "auto", "broad", 0, 100),
    (4096, 7, "sum4", "FULL", "amplitude", True, 8, 1, (6.0, 1.5), "seq_mad_cm", "specials", 16, 110),
    (9100, 31, "sum8", "CHANNEL", "complex", True, 11, 128, (11.0, 1.2), "seq_madt_cm", "ties", 16, 120),
    (13000, 3, "sum1", "CHANNEL", "amplitude", False, 17, 1, (11.0, 1.2), "seq_madt_t", "sparse", 0, 130),
    (700, 13, "sum6", "FULL", "complex", False, 8, 128, (11.0, 1.2), "seq_mad_t", "specials", 0, 140),
    (40, 21, "simple", "NONE", "amplitude", True, 17, 1, (6.0, 1.5), "seq_mad_t", "ties", 16, 150),
    (200, 13, "sum6", "CHANNEL", "amplitude", True, 11, 1, (6.0, 1.5), "auto", "broad", 16, 160),
    (3000, 21, "sum4", "NONE", "complex", False, 11, 128, (11.0, 1.2), "seq_mad_cm", "sparse", 0, 170),
    (700, 31, "sum1", "FULL", "amplitude", True, 3, 1, (6.0, 1.5), "seq_madt_cm", "sparse", 16, 180),
    (200, 7, "sum8", "FULL", "complex", False, 17, 128, (6.0, 1.5), "seq_madt_t", "ties", 0, 190),
    (3000, 63, "simple", "CHANNEL", "amplitude", True, 8, 1, (11.0, 1.2), "seq_madt_t", "specials", 16, 200),
    (40, 3, "sum1", "FULL", "complex", True, 8, 128, (11.0, 1.2), "auto", "broad", 0, 210),
    (4096, 31, "sum6", "NONE", "complex", False, 17, 1, (11.0, 1.2), "seq_madt_cm", "specials", 0, 220),
    (5000, 3, "sum4", "CHANNEL", "amplitude", True, 3, 1, (11.0, 1.2), "seq_mad_t", "ties", 16, 230),
    (9100, 3, "sum8", "NONE", "amplitude", False, 8, 1, (6.0, 1.5), "auto", "specials", 0, 240),
    (13000, 7, "sum1", "NONE", "amplitude", True, 11, 128, (6.0, 1.5), "seq_mad_t", "specials", 16, 250),
    (700, 63, "sum8", "CHANNEL", "complex", False, 17, 128, (11.0, 1.2), "seq_mad_cm", "broad", 16, 260),
    (40, 7, "sum6", "CHANNEL", "complex", False, 3, 1, (6.0, 1.5), "seq_madt_t", "sparse", 0, 270),
    (13000, 13, "simple", "FULL", "complex", False, 3, 128, (11.0, 1.2), "seq_mad_cm", "ties", 0, 280),
    (4096, 21, "sum8", "CHANNEL", "amplitude", False, 3, 128, (6.0, 1.5), "auto", "sparse", 16, 290),
    (9100, 13, "sum4", "NONE", "complex", True, 17, 1, (6.0, 1.5), "seq_madt_t", "sparse", 16, 300),
    (13000, 21, "sum4", "FULL", "amplitude", True, 8, 1, (11.0, 1.2), "seq_madt_cm", "broad", 0, 310),
    (200, 31, "simple", "NONE", "amplitude", False, 8, 128, (11.0, 1.2), "seq_mad_t", "sparse", 0, 320),
    (3000, 63, "sum6", "FULL", "amplitude", False, 11, 128, (6.0, 1.5), "seq_madt_cm", "ties", 16, 330),
    (700, 7, "simple", "NONE", "complex", True, 11, 128, (11.0, 1.2), "seq_madt_t", "broad", 0, 340),
    (5000, 21, "sum1", "FULL", "amplitude", True, 3, 1, (11.0, 1.2), "seq_mad_cm", "specials", 16, 350),
    (9100, 63, "sum1", "FULL", "complex", False, 3, 128, (6.0, 1.5), "seq_mad_t", "broad", 16, 360),
    (3000, 31, "sum4", "FULL", "amplitude", True, 17, 128, (11.0, 1.2), "auto", "broad", 0, 370),
    (4096, 3, "simple", "CHANNEL", "complex", True, 11, 128, (11.0, 1.2), "seq_madt_cm", "ties", 16, 380),
    (5000, 13, "sum8", "FULL", "complex", False, 8, 128, (11.0, 1.2), "seq_madt_cm", "sparse", 0, 390),
    (200, 3, "sum6", "FULL", "complex", True, 3, 128, (6.0, 1.5), "seq_mad_cm", "specials", 16, 400),
    (700, 21, "sum4", "NONE", "complex", True, 8, 1, (11.0, 1.2), "auto", "ties", 0, 410),
    (40, 63, "sum4", "FULL", "amplitude", True, 11, 128, (11.0, 1.2), "seq_madt_cm", "specials", 16, 420),
    (3000, 13, "sum1", "FULL", "amplitude", True, 3, 128, (6.0, 1.5), "seq_mad_t", "ties", 16, 430),
    (5000, 21, "sum6", "NONE", "amplitude", True, 11, 128, (6.0, 1.5), "seq_madt_t", "sparse", 16, 440),
    (40, 31, "sum8", "CHANNEL", "complex", True, 8, 1, (11.0, 1.2), "seq_mad_cm", "specials", 0, 450),
    (4096, 63, "sum8", "FULL", "amplitude", False, 8, 128, (11.0, 1.2), "seq_mad_t", "sparse", 0, 460),
    (4096, 13, "sum1", "FULL", "amplitude", False, 8, 128, (6.0, 1.5), "seq_madt_t", "broad", 0, 470),
    (9100, 21, "sum6", "FULL", "amplitude", False, 8, 1, (6.0, 1.5), "seq_mad_cm", "specials", 0, 480),
    (5000, 7, "sum4", "NONE", "amplitude", True, 17, 128, (11.0, 1.2), "auto", "specials", 16, 490),
    (13000, 31, "sum8", "NONE", "amplitude", True, 3, 1, (6.0, 1.5), "auto", "specials", 0, 500),
    (9100, 7, "simple", "FULL", "complex", False, 11, 1, (11.0, 1.2), "seq_madt_cm", "broad", 0, 510),
    (200, 21, "sum1", "CHANNEL", "amplitude", True, 17, 128, (11.0, 1.2), "seq_madt_cm", "sparse", 16, 520),
    (3000, 7, "sum8", "FULL", "amplitude", True, 3, 128, (11.0, 1.2), "seq_mad_t", "sparse", 16, 530),
    (200, 63, "sum4", "NONE", "complex", False, 17, 1, (11.0, 1.2), "seq_madt_cm", "sparse", 16, 540),
    (5000, 31, "sum4", "FULL", "amplitude", False, 3, 1, (6.0, 1.5), "seq_madt_t", "ties", 16, 550),
    (13000, 63, "sum6", "FULL", "complex", False, 3, 1, (11.0, 1.2), "seq_mad_cm", "specials", 0, 560),
    (3000, 3, "sum8", "NONE", "amplitude", True, 8, 128, (6.0, 1.5), "seq_mad_cm", "ties", 16, 570),
    (40, 13, "sum1", "FULL", "amplitude", True, 11, 1, (6.0, 1.5), "seq_madt_t", "ties", 0, 580),
    (700, 3, "sum4", "CHANNEL", "complex", True, 3, 1, (11.0, 1.2), "auto", "sparse", 0, 590),
)

FUSED_CLASSES = (
    # 4 channels per lane (width 13, up to 256 channels, at most 4 windows)
    (200, 13, "simple", "FULL", "amplitude", False, 11, 128, (6.0, 1.5), "auto", "ties", 16, 600),
    (200, 13, "sum4", "CHANNEL", "complex", True, 17, 1, (11.0, 1.2), "auto", "specials", 0, 610),
    # 16 channels per lane (width 13, up to 1024 channels, at most 4 windows)
    (700, 13, "sum4", "FULL", "amplitude", True, 17, 128, (6.0, 1.5), "auto", "broad", 16, 620),
    (700, 13, "simple", "CHANNEL", "complex", False, 3, 1, (11.0, 1.2), "auto", "specials", 0, 630),
    # 64 channels per lane: beyond 1024 channels, another width, or more than 4 windows
    (3000, 13, "sum1", "CHANNEL", "amplitude", False, 11, 128, (11.0, 1.2), "auto", "ties", 0, 640),
    (3000, 21, "simple", "FULL", "amplitude", True, 17, 1, (6.0, 1.5), "auto", "specials", 16, 650),
    (3000, 7, "sum6", "CHANNEL", "amplitude", True, 8, 128, (6.0, 1.5), "auto", "broad", 0, 660),
    (4096, 13, "sum8", "NONE", "complex", False, 11, 128, (6.0, 1.5), "auto", "broad", 0, 670),
    (4096, 13, "sum4", "FULL", "complex", True, 8, 1, (11.0, 1.2), "auto", "sparse", 16, 680),
    (4096, 13, "sum4", "NONE", "amplitude", False, 17, 1, (6.0, 1.5), "auto", "ties", 0, 690),
    # long bands in strips of 4 baselines (4097 .. 9088 channels)
    (5000, 13, "sum4", "FULL", "amplitude", True, 11, 128, (6.0, 1.5), "auto", "broad", 16, 700),
    (5000, 13, "simple", "CHANNEL", "complex", False, 17, 1, (11.0, 1.2), "auto", "specials", 0, 710),
    # long bands in strips of 3 baselines (9089 .. 12288 channels)
    (9100, 13, "simple", "FULL", "amplitude", False, 17, 128, (11.0, 1.2), "auto", "ties", 16, 720),
    (9100, 13, "sum4", "NONE", "complex", True, 8, 1, (6.0, 1.5), "auto", "specials", 0, 730),
)

RING = (
    (4096, 13, "sum4", "NONE", "complex", False, 8, 1, (11.0, 1.2), "auto", "sparse", 0, 800),
    (4096, 13, "simple", "NONE", "complex", False, 11, 128, (6.0, 1.5), "auto", "broad", 16, 810),
    (4096, 13, "sum1", "NONE", "complex", False, 17, 1, (6.0, 1.5), "auto", "ties", 0, 820),
    (4096, 13, "sum4", "NONE", "complex", False, 17, 128, (11.0, 1.2), "auto", "specials", 16, 830),
    (4096, 13, "simple", "NONE", "complex", False, 8, 128, (11.0, 1.2), "auto", "specials", 0, 840),
    (4096, 13, "sum1", "NONE", "complex", False, 11, 1, (11.0, 1.2), "auto", "broad", 16, 850),
    (4096, 13, "sum4", "NONE", "complex", False, 11, 128, (6.0, 1.5), "auto", "ties", 0, 860),
)
# fmt: on

PAIRWISE_CASES = tuple(Case(*row) for row in PAIRWISE)
FUSED_CLASS_CASES = tuple(Case(*row) for row in FUSED_CLASSES)
RING_CASES = tuple(Case(*row) for row in RING)
CASES = PAIRWISE_CASES + FUSED_CLASS_CASES + RING_CASES

MADT_MAX_CHANNELS = 16384  # of the NoiseEstMADT template: beyond the longest band of the table


def all_pairs():
    """Every (factor, level, factor, level) of two different factors of :data:`FACTORS`."""
    for (i, (_, levels_i)), (j, (_, levels_j)) in itertools.combinations(enumerate(FACTORS), 2):
        for a in levels_i:
            for b in levels_j:
                yield i, a, j, b


def pairs_of(case):
    """The pairs of :func:`all_pairs` that `case` covers."""
    return {(i, case[i], j, case[j]) for i, j in itertools.combinations(range(len(FACTORS)), 2)}


# ------------------------------------------------ the dispatch, from its documented conditions
def documented_fusable(case):
    """Do the fused kernels take this case's stages and size? Written from the documentation
    of the dispatch (not by calling the library): median widths 3 .. 31 and 1 .. 8 windows
    up to 4096 channels; beyond, up to 12288 channels, width 13 and at most 4 windows."""
    if case.channels <= 4096:
        return case.width <= 31 and case.n_windows <= 8
    return case.channels <= 12288 and case.width == 13 and case.n_windows <= 4


def runs_fused(case):
    return not case.forced_sequence and documented_fusable(case)


def ring_eligible(case):
    """The persistent ring kernel's conditions: a fused launch of 4096 channels of complex
    visibilities, no mask, width 13, no deviations, at most 4 windows, at least 8 baselines."""
    return (runs_fused(case) and case.channels == 4096 and not case.amplitudes
            and case.mask == "NONE" and case.width == 13 and not case.keep_deviations
            and case.n_windows <= 4 and case.baselines >= 8)  # fmt: skip


def kernel_class(case, ring_allowed=True):
    """Which flagger runs the case: ``sequence``, ``ring`` (only where `ring_allowed`: the ring
    kernel is otherwise chosen by size, from far more baselines than the table has), ``long4``
    and ``long3`` (long bands in strips of 4 or 3 baselines), or ``strip4``, ``strip16`` and
    ``strip64`` by the channels a lane owns (4 and 16 need width 13 and at most 4 windows)."""
    if not runs_fused(case):
        return "sequence"
    if ring_allowed and ring_eligible(case):
        return "ring"
    if case.channels > 4096:
        return "long4" if case.channels <= 9088 else "long3"
    if case.width != 13 or case.n_windows > 4 or case.channels > 1024:
        return "strip64"
    return "strip4" if case.channels <= 256 else "strip16"


# ----------------------------------------------------------------------------------- inputs
def _sparse(case):
    vis = inputs.generate_data(case.channels, case.baselines, seed=case.seed)
    return inputs.add_rfi(vis, seed=case.seed + 1, fraction=0.08)


def _broad(case):
    """Runs of 1 to 120 channels scaled by 2 to 4 and a few spikes: what the wider windows of
    SumThreshold fire on and the narrow ones do not. A run longer than the median filter
    raises the background with it, so half of the runs raise every second channel only. Two
    more structures give every window its turn:

    * bands of 200 channels and more carry, in their lower half, a comb on channels 0 and 2 of
      every 5 whose carrier grows from 0 to 8 (some 10 times the noise) along up to 600
      channels: with 6 sigma and a falloff of 1.5 each window in turn, the widest first, is the
      first to reach its threshold somewhere on that ramp;
    * with 11 sigma and a falloff of 1.2 the window of 128 channels asks for a mean of 3.07
      times the noise where that of 64 asks for 3.68 and a single sample for 11, which noise
      of the usual level hardly ever leaves room for. Bands of 700 channels and more therefore
      have, in their upper half, a quiet stretch (a fifth of the noise) of up to 400 channels
      in which every third channel carries 8 to 10.45, a level per baseline: about 10 times
      the noise estimate, a mean of about 3.3 over any window."""
    channels, baselines = case.channels, case.baselines
    rs = np.random.RandomState(case.seed + 2)
    vis = inputs.generate_data(channels, baselines, seed=case.seed)
    longest = min(120, channels // 4)
    half = channels // 2
    for b in range(baselines):
        for _ in range(2 + channels // 1000):
            length = rs.randint(1, longest + 1)
            start = rs.randint(0, channels - length + 1)
            step = rs.randint(1, 3)
            vis[start : start + length : step, b] *= np.float32(rs.uniform(2.0, 4.0))
        if channels >= 200:
            length = min(600, channels // 3)
            start = rs.randint(0, half - length + 1)
            ramp = 8.0 * np.cbrt(np.linspace(0.0, 1.0, length)) * np.exp(2j * np.pi * rs.rand())
            for first in (0, 2):
                vis[start + first : start + length : 5, b] += ramp[first::5].astype(np.complex64)
        if channels >= 700:
            length = min(400, channels // 3)
            start = half + rs.randint(0, channels - half - length + 1)
            vis[start : start + length, b] *= np.float32(0.2)
            vis[start : start + length : 3, b] += np.float32(8.0 + 0.35 * (b % 8))
        vis[rs.randint(0, channels, 3), b] *= np.float32(rs.uniform(20.0, 60.0))
    return vis


def _ties(case):
    """Real amplitudes on a grid of 1/8 (crowded MAD bins, even and odd counts of equal
    deviations), plus spikes."""
    vis = inputs.generate_data(case.channels, case.baselines, seed=case.seed)
    vis = (np.round(vis.real * 8.0) / 8.0).astype(np.complex64)
    return inputs.add_rfi(vis, seed=case.seed + 1, fraction=0.04)


def _specials(case):
    """Sparse interference, an all-zero baseline, a constant one, and in the last baseline one
    each of inf, NaN, a finite value whose |z| overflows, and a subnormal."""
    vis = _sparse(case)
    channels = case.channels
    vis[:, 0] = 0
    vis[:, 1] = 3 + 4j
    last = case.baselines - 1
    vis[channels // 5, last] = np.inf
    vis[2 * channels // 5, last] = complex(np.nan, 0.0)
    vis[3 * channels // 5, last] = complex(3e38, 3e38)
    vis[4 * channels // 5, last] = np.float32(1e-42)
    return vis


_DATA = {"sparse": _sparse, "broad": _broad, "ties": _ties, "specials": _specials}


@functools.lru_cache(maxsize=None)
def make_vis(case):
    """complex64 visibilities [channels][baselines] of the case's data class (read-only)."""
    vis = _DATA[case.data](case)
    assert vis.dtype == np.complex64 and vis.shape == (case.channels, case.baselines)
    vis.setflags(write=False)
    return vis


@functools.lru_cache(maxsize=None)
def make_input(case):
    """What the flagger is given: the visibilities, or their amplitudes (numpy's float32 |z|)."""
    vis = make_vis(case)
    if not case.amplitudes:
        return vis
    from oracle import rfi_oracle

    with np.errstate(all="ignore"):
        amp = rfi_oracle.abs_c64(vis)
    amp.setflags(write=False)
    return amp


@functools.lru_cache(maxsize=None)
def make_mask(case):
    """``None``, a CHANNEL mask (1/8 of the channels, value 4) or a FULL mask (0.15 of the
    samples with values 2 and 6, and channels 20 .. 39 masked on every baseline with 1 where
    the band is longer than that, so that some windows have no valid sample)."""
    rs = np.random.RandomState(case.seed + 3)
    if case.mask == "NONE":
        return None
    if case.mask == "CHANNEL":
        mask = (rs.random_sample(case.channels) < 1.0 / 8.0).astype(np.uint8) * np.uint8(4)
    else:
        shape = (case.channels, case.baselines)
        mask = (rs.random_sample(shape) < 0.15).astype(np.uint8)
        mask *= rs.choice(np.array([2, 6], np.uint8), size=shape)
        if case.channels > 40:
            mask[20:40, :] = 1
    mask.setflags(write=False)
    return mask


# ------------------------------------------------------------------------------- references
def oracle_kwargs(case, n_windows=None):
    kw = dict(width=case.width, amplitudes=case.amplitudes, n_sigma=case.n_sigma,
              flag_value=case.flag_value, threshold="sum" if case.sum_threshold else "simple")  # fmt: skip
    if case.sum_threshold:
        kw.update(n_windows=case.n_windows if n_windows is None else n_windows,
                  threshold_falloff=case.threshold_falloff)  # fmt: skip
    return kw


@functools.lru_cache(maxsize=None)
def reference(case):
    """(flags, noise float64, deviations float64) of ``oracle.flagger_full``: what the fused
    kernels and ``rfi.host.FlaggerHost`` must reproduce."""
    from oracle import rfi_oracle

    with np.errstate(all="ignore"):
        return rfi_oracle.flagger_full(make_input(case), make_mask(case), want_deviations=True,
                                       **oracle_kwargs(case))  # fmt: skip


def reference_flags(case, masked=True, n_windows=None):
    """The oracle's flags without the mask, or with another number of windows."""
    from oracle import rfi_oracle

    with np.errstate(all="ignore"):
        return rfi_oracle.flagger_full(make_input(case), make_mask(case) if masked else None,
                                       **oracle_kwargs(case, n_windows))[0]  # fmt: skip


def threshold_oracle(case):
    from oracle import rfi_oracle

    if case.sum_threshold:
        return rfi_oracle.ThresholdSumHost(case.n_sigma, case.n_windows, case.threshold_falloff,
                                           case.flag_value)  # fmt: skip
    return rfi_oracle.ThresholdSimpleHost(case.n_sigma, case.flag_value)


@functools.lru_cache(maxsize=None)
def staged_reference(case):
    """(flags, noise float32, deviations float32) of the oracle's stages chained through
    float32 intermediates, which is what the separate device buffers of the kernel-per-stage
    sequence imply."""
    from oracle import rfi_oracle

    with np.errstate(all="ignore"):
        dev32 = rfi_oracle.BackgroundMedianFilterHost(case.width, case.amplitudes)(
            make_input(case), make_mask(case)).astype(np.float32)  # fmt: skip
        noise32 = rfi_oracle.NoiseEstMADHost()(dev32).astype(np.float32)
        flags = threshold_oracle(case)(dev32, noise32)
    return flags, noise32, dev32
