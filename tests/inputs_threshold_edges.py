"""Flagger inputs whose window sums (SumThreshold) or samples (simple threshold) lie on their
limit so closely that float32 deviations decide them wrongly. NumPy and ``rfi.host`` only.

The host's rule is a float64 one: deviations are ``amplitude - median`` in float64, a window of
``w = 2**k`` channels fires when its sequential float64 sum exceeds ``float32(thr_k * w)``, and
samples flagged by earlier windows stand in as exactly ``thr_k``. The fused kernels keep float32
deviations and go back to exact ones only for windows within an error bound of the limit. Every
planted window here is such a window, and is decided *differently* by the host from float64
deviations and from ``deviations.astype(float32)`` -- a kernel that decided it from float32
values alone, or re-summed the wrong channels, gets it wrong.

How a column is built (amplitudes; the complex form has a zero imaginary part, so ``|z|`` is exact):

* quiet channels are ``m``, every fifth one ``m - 0.25``: every median is ``m``, every quiet
  deviation an exact dyadic (0 or -0.25), and the MAD noise ``1.4826 * 0.25`` in every baseline;
* direction ``exact`` (the exact rule fires, float32 does not): ``m = 1 - 3 * 2**-24``; a *big*
  sample 65.0 deviates by ``64 + 3 * 2**-24``, which float32 rounds to 64.0. A window holding
  ``n`` of them (and zeros) sums to ``64 n + 3 n 2**-24`` against the limit ``64 n``;
* direction ``float32`` (float32 fires, the exact rule does not): ``m = 1 + 2**-23``; a big
  sample deviates by ``64 - 2**-23`` (float32: 64.0), and a *tick* sample ``m + n * 2**-23``
  -- another binade, so its deviation ``n * 2**-23`` is exact in float32 -- brings the exact sum
  to the limit ``64 n`` itself (a tie: no flag), the float32 one to ``64 n + n * 2**-23``.
  Window 1 has no such case: its threshold is a float32 and rounding is monotone, so
  ``float32(d) > thr`` implies ``d > thr``. ``DIRECTIONS`` says so;
* ``replaced``: ``w - 1`` samples of 1001.0, which window 1 flags, and then one big sample:
  the flagged ones count as exactly ``thr_k = 64``, the big one decides (direction ``exact``);
* the simple threshold: one big sample, ``n_sigma * noise`` (float64) strictly between its exact
  deviation and 64.0, from either side.

Windows of one and two channels (direction ``exact``) and the replaced ones use the default
falloff 1.2. Everything else uses 2.0, with which ``w * thr_k`` is the same for every window size,
so that no smaller window holding fewer big samples fires first; the big samples sit at the first,
the middle and the last channel of the window, so no shifted window holds them all.

``n_sigma`` is found with ``nextafter`` steps so that ``float32(n_sigma * noise * falloff**-k)``
is the intended float32. ``check_premises`` asserts all of it with ``rfi.host`` -- conditions, not
measurements -- and every case is checked before it is returned.
"""

import dataclasses
import functools
import os
from typing import List, Optional, Tuple

import numpy as np

from katsdpsigproc_amd.rfi import host

Q = np.float32(0.25)
M_EXACT = np.float32(1.0 - 3 * 2.0**-24)
M_FLOAT32 = np.float32(1.0 + 2.0**-23)
BIG = np.float32(65.0)
HUGE = np.float32(1001.0)
GAP = 32  # quiet channels between planted windows: no median window (<= 31) sees two of them

#: the reference's own flags for the cases of at most 4096 channels
#: (tests/golden/make_golden_threshold_edges.py)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "rfi_host_threshold_edges_golden.npz")  # fmt: skip
GOLDEN_MAX_CHANNELS = 4096
GOLDEN_PACKED_CHANNELS = 320  # flags stored bit for bit up to here, as a digest beyond

#: which (window, direction) pairs exist; window 1 of SumThreshold has no "float32" direction
DIRECTIONS = {w: (("exact",) if w == 1 else ("exact", "float32")) for w in (1, 2, 4, 8, 16, 32, 64, 128)}
#: windows for which a "replaced" case is built, by median width (w - 1 + 1 samples above the
#: median must stay a minority of every median window)
REPLACED = {13: (2, 4), 31: (2, 4, 8)}

#: path -> (shapes, windows). The shapes are the smallest that reach the path.
PATHS = {
    "fused4": (((320, 5), (4096, 5)), (1, 2, 4, 8, 16, 32, 64, 128)),
    "ring": (((4096, 8), (4096, 12)), (1, 2, 4, 8)),
    "long": (((8192, 3), (10240, 3)), (1, 2, 4, 8)),
}


@dataclasses.dataclass
class Case:
    name: str
    path: str
    kind: str  # "sum" or "simple"
    direction: str  # "exact": only the exact rule fires; "float32": only float32 does
    window: int
    replaced: bool
    vis: np.ndarray  # complex64 with zero imaginary part, or float32 if `amplitudes`
    amplitudes: bool
    width: int
    n_sigma: float
    n_windows: int
    threshold_falloff: float
    keep_deviations: bool
    in_flags: Optional[np.ndarray]  # per-channel mask (flag mode CHANNEL) or None
    planted: List[Tuple[int, int, int]]  # (baseline, first channel, w)
    target: Optional[np.float32]  # intended float32(thr_k) of the planted window size (sum)

    @property
    def threshold(self):
        if self.kind == "simple":
            return host.ThresholdSimpleHost(self.n_sigma)
        return host.ThresholdSumHost(self.n_sigma, self.n_windows, self.threshold_falloff)

    def host_stages(self):
        """(float64 deviations, noise, flags of the exact rule, flags from float32 deviations)."""
        bg = host.BackgroundMedianFilterHost(self.width, self.amplitudes)
        dev = bg(self.vis) if self.in_flags is None else bg(self.vis, self.in_flags)
        noise = host.NoiseEstMADHost()(dev)
        thr = self.threshold
        return dev, noise, thr(dev, noise), thr(dev.astype(np.float32), noise)


def _roles(w: int, direction: str, replaced: bool):
    """[(offset in the window, role)], and the number of big samples that decide the sum."""
    if replaced:
        return [(i, "huge") for i in range(w - 1)] + [(w - 1, "big")], 1
    if w == 1:
        return [(0, "big")], 1
    if w == 2:
        return ([(0, "big"), (1, "big")], 2) if direction == "exact" else ([(0, "big"), (1, "tick")], 1)
    mid = "big" if direction == "exact" else "tick"
    return [(0, "big"), (w // 2, mid), (w - 1, "big")], (3 if direction == "exact" else 2)


def _straddles(w: int):
    """How many channels of a window lie before a lane boundary."""
    return list(range(1, w)) if w <= 8 else [1, w // 2, w - 1]


def _boundary_straddles(w: int):
    """The same across a boundary between two kernels' segments: one window per baseline can
    cross it, and the long-band kernels are tested with 3 baselines."""
    return sorted({1, w // 2, w - 1} - {0})


def _place(channels: int, baselines: int, w: int, boundaries=(), ends=True):
    """First channels (baseline, c) of the planted windows: the first and the last w channels of
    the band, across every boundary of `boundaries` and across lane boundaries (64 L - j for each
    j of ``_straddles``), and inside a lane's run of 64; round robin over the baselines so that
    every position of a strip of 4 or 8, and a last partial strip, holds some. ValueError if one
    of these kinds finds no room. Without `ends` the band's ends are left out: the median window
    of the band's first or last channel is clipped to half its width, 7 channels of 13, and must
    hold fewer than 4 planted samples."""
    taken = [[] for _ in range(baselines)]
    placed = []
    kinds = set()

    def put(kind, c, start, only=False):
        if c < 0 or c + w > channels:
            return False
        for k in range(1 if only else baselines):
            b = (start + k) % baselines
            if all(c + w + GAP <= lo or hi + GAP <= c for lo, hi in taken[b]):
                taken[b].append((c, c + w))
                placed.append((b, c, w))
                kinds.add(kind)
                return True
        return False

    n = 0
    for c in (0, channels - w) if ends else ():
        for b in (0, baselines - 1):  # (both ends in the first and in the last baseline)
            put("first" if c == 0 else "last", c, b)
    for boundary in boundaries:
        for j in _boundary_straddles(w):
            n += put(("boundary", boundary, j), boundary - j, n % baselines)
    lanes = channels // 64
    if w <= 32:
        for i in range(baselines):
            put("inside", 64 * ((5 * i + 2) % lanes) + 20, i)
    lane = 1
    # (three lane boundaries per straddle, spread over the band; one in a short band)
    for _ in range(3 if lanes >= 16 else 1):
        for j in _straddles(w):
            for _try in range(lanes):
                lane = lane % (lanes - 1) + 1 if lanes > 1 else 1
                if put(("straddle", j), 64 * lane - j, n % baselines):
                    n += 1
                    break
    for b in range(baselines):  # (a baseline left empty so far: any straddle that fits)
        if not taken[b]:
            any(put(("straddle", j), 64 * ln - j, b, only=True)
                for ln in range(1, lanes) for j in (_straddles(w) or [0]))
    want = {"first", "last"} | {("boundary", b, j) for b in boundaries for j in _boundary_straddles(w)}
    want |= {("straddle", j) for j in _straddles(w)}
    if w <= 32:
        want.add("inside")
    if not ends:
        want -= {"first", "last"}
    if want - kinds:
        raise ValueError(f"no room for {sorted(map(str, want - kinds))} at {channels} x {baselines}, w={w}")
    if {b for b, _, _ in placed} != set(range(baselines)):
        raise ValueError(f"a baseline without a planted window at {channels} x {baselines}, w={w}")
    return sorted(placed)


def _aim_sum(noise: float, scale: float, target: np.float32) -> float:
    """n_sigma with ``float32(n_sigma * noise * scale) == target``, as the host rounds it."""
    n = float(target) / (noise * scale)
    for _ in range(1000):
        got = np.float32((n * noise) * scale)
        if got == target:
            return n
        n = float(np.nextafter(n, np.inf if got < target else -np.inf))
    raise ValueError(f"no n_sigma gives the threshold {target!r}")


def _aim_simple(noise: float, lo: float, hi: float) -> float:
    """n_sigma with ``lo < n_sigma * noise < hi`` in float64."""
    n = (lo + hi) / 2 / noise
    for _ in range(1000):
        got = n * noise
        if lo < got < hi:
            return n
        n = float(np.nextafter(n, np.inf if got <= lo else -np.inf))
    raise ValueError(f"no n_sigma puts the threshold inside ({lo!r}, {hi!r})")


def _build(name, path, shape, kind, w, direction, replaced, *, width=13, n_windows=4,
           amplitudes=False, keep_deviations=False, masked=False, boundaries=()) -> Case:  # fmt: skip
    channels, baselines = shape
    m = M_EXACT if direction == "exact" else M_FLOAT32
    roles, n_big = _roles(w, direction, replaced)
    tick = np.float32(float(M_FLOAT32) + n_big * 2.0**-23)  # (direction "float32" only)
    assert float(tick) == float(M_FLOAT32) + n_big * 2.0**-23
    amp = np.full(shape, m, np.float32)
    amp[::5] = m - Q
    assert float(amp[0, 0]) == float(m) - 0.25  # (exact: the quiet deviations are dyadic)
    planted = _place(channels, baselines, w, boundaries, ends=len(roles) < 4)
    for b, c, _ in planted:
        amp[c : c + w, b] = m
        for off, role in roles:
            amp[c + off, b] = {"big": BIG, "huge": HUGE, "tick": tick}[role]
    in_flags = None
    if masked:
        # masked channels, each at least GAP away from every planted window
        near = np.zeros(channels, bool)
        for _, c, _ in planted:
            near[max(0, c - GAP) : c + w + GAP] = True
        free = np.flatnonzero(~near)
        in_flags = np.zeros(channels, np.uint8)
        in_flags[free[3::11]] = 1
        if not in_flags.any():
            raise ValueError(f"{name}: no room for masked channels")
    noise = float(host.MAD_NORMAL) * 0.25
    if kind == "simple":
        falloff, n_windows, target = 1.2, 1, None
        exact = 64.0 + 3 * 2.0**-24 if direction == "exact" else 64.0 - 2.0**-23
        n_sigma = _aim_simple(noise, min(exact, 64.0), max(exact, 64.0))
    else:
        falloff = 1.2 if replaced or (direction == "exact" and w <= 2) else 2.0
        target = np.float32(64.0 if replaced else 64.0 * n_big / w)
        k = w.bit_length() - 1
        if k >= n_windows:
            raise ValueError(f"{name}: window {w} needs more than {n_windows} windows")
        n_sigma = _aim_sum(noise, pow(falloff, -k), target)
    vis = amp if amplitudes else amp.astype(np.complex64)
    vis.setflags(write=False)
    case = Case(name, path, kind, direction, w, replaced, vis, amplitudes, width, n_sigma,
                n_windows, falloff, keep_deviations, in_flags, planted, target)  # fmt: skip
    check_premises(case)
    return case


def check_premises(case: Case) -> int:
    """Assert, with ``rfi.host``, that `case` is what it claims to be; returns the number of
    discriminating windows."""
    dev, noise, exact, rounded = case.host_stages()
    tag = case.name
    assert np.all(noise == float(host.MAD_NORMAL) * 0.25), f"{tag}: noise is not 1.4826 * 0.25"
    k = case.window.bit_length() - 1
    if case.kind == "sum":
        # the threshold is what was aimed at
        thr = (case.n_sigma * noise * pow(case.threshold_falloff, -k)).astype(np.float32)
        assert np.all(thr == case.target), f"{tag}: thr_{k} = {thr!r}, not {case.target!r}"
    expected = np.zeros(dev.shape, np.uint8)
    for b, c, w in case.planted:
        assert w == case.window and 0 <= c and c + w <= dev.shape[0]
        decider = c + w - 1 if case.replaced else c
        d = dev[decider, b]
        assert float(np.float32(d)) == 64.0 and d != 64.0, f"{tag}: deviation {d!r}"
        assert (d > 64.0) == (case.direction == "exact")
        if case.kind == "simple":
            limit = case.n_sigma * noise[b]
            assert min(d, 64.0) < limit < max(d, 64.0), f"{tag}: limit {limit!r} vs {d!r}"
        win = (slice(c, c + w), b)
        mine, other = (exact, rounded) if case.direction == "exact" else (rounded, exact)
        assert mine[win].all(), f"{tag}: window at {c} of baseline {b} does not fire"
        if case.replaced:  # (the samples window 1 flagged are flagged either way)
            assert other[c : c + w - 1, b].all() and not other[decider, b]
        else:
            assert not other[win].any(), f"{tag}: window at {c} of baseline {b} fires either way"
        if case.direction == "exact":
            expected[win] = 1
        elif case.replaced:
            expected[c : c + w - 1, b] = 1
    # the planted windows are all there is: nothing else is flagged, nothing else is close
    assert np.array_equal(exact, expected), f"{tag}: flags outside the planted windows"
    if case.in_flags is not None:
        masked = np.flatnonzero(case.in_flags)
        for _, c, w in case.planted:
            assert np.all((masked < c - case.width) | (masked >= c + w + case.width))
    strips = {b % 4 for b, _, _ in case.planted}
    assert strips == set(range(min(4, dev.shape[1]))), f"{tag}: strip positions {strips}"
    return len(case.planted)


def _variants(path: str, i: int, channels: int) -> dict:
    """Settings the issue's table varies on the 4-baseline kernel, dealt out over the cases so
    that every value meets several window sizes; the other paths have one setting."""
    if path == "fused4":
        return dict(width=31 if i % 3 == 1 else 13, amplitudes=bool(i % 2),
                    keep_deviations=bool((i // 2) % 2),
                    masked=i % 4 == 3 and channels > 320)  # fmt: skip
        # (320 channels have no room for masked channels away from the windows of 5 baselines)
    if path == "long":
        return dict(amplitudes=bool(i % 2))
    return {}


@functools.lru_cache(maxsize=None)
def cases(path: str) -> Tuple[Case, ...]:
    """Every case of `path` ("fused4", "ring" or "long"), premises checked. A (path, window,
    direction) combination that cannot be produced raises instead of being left out."""
    shapes, windows = PATHS[path]
    out = []
    for shape in shapes:
        channels = shape[0]
        boundaries = tuple(b for b in (4096, 8192) if b < channels) if path == "long" else ()
        i = len(out)
        for w in windows:
            # (4, 5, 6, 7, 8: the planted size is the largest beyond 8 channels, or a larger
            # window would hold samples of two planted ones)
            n_windows = max(4, w.bit_length())
            for direction in DIRECTIONS[w]:
                opts = _variants(path, i, channels)
                out.append(_build(f"{path}_{channels}x{shape[1]}_sum_w{w}_{direction}", path, shape,
                                  "sum", w, direction, False, n_windows=n_windows,
                                  boundaries=boundaries, **opts))  # fmt: skip
                i += 1
        widths = (13, 31) if path == "fused4" else (13,)
        for width in widths:
            for w in REPLACED[width]:
                if width == 31 and w < 8:
                    continue  # (width 13 has them)
                opts = dict(_variants(path, i, channels), width=width)
                out.append(_build(f"{path}_{channels}x{shape[1]}_sum_w{w}_replaced", path, shape,
                                  "sum", w, "exact", True, boundaries=boundaries, **opts))  # fmt: skip
                i += 1
        for direction in ("exact", "float32"):
            opts = _variants(path, i, channels)
            out.append(_build(f"{path}_{channels}x{shape[1]}_simple_{direction}", path, shape,
                              "simple", 1, direction, False, boundaries=boundaries, **opts))  # fmt: skip
            i += 1
    return tuple(out)


def all_cases() -> Tuple[Case, ...]:
    return tuple(case for path in PATHS for case in cases(path))


def names(path: str) -> List[str]:
    """The case names of `path`, without building anything (for parametrising tests)."""
    shapes, windows = PATHS[path]
    out = []
    for channels, baselines in shapes:
        stem = f"{path}_{channels}x{baselines}"
        out += [f"{stem}_sum_w{w}_{d}" for w in windows for d in DIRECTIONS[w]]
        for width in (13, 31) if path == "fused4" else (13,):
            out += [f"{stem}_sum_w{w}_replaced" for w in REPLACED[width] if width == 13 or w >= 8]
        out += [f"{stem}_simple_exact", f"{stem}_simple_float32"]
    return out


def by_name(name: str) -> Case:
    path = name.split("_", 1)[0]
    for case in cases(path):
        if case.name == name:
            return case
    raise KeyError(name)


#: (path, shape, w, width) of ``band_end_case``: 3 big samples fit the clipped median window of
#: width 13 at the band's end (7 channels), 7 fit that of width 31 (16 channels)
BAND_END = [
    ("fused4", (320, 5), 4, 13), ("fused4", (320, 5), 8, 31), ("fused4", (4096, 5), 4, 13),
    ("fused4", (4096, 5), 8, 31), ("ring", (4096, 8), 4, 13), ("ring", (4096, 12), 4, 13),
    ("long", (8192, 3), 4, 13), ("long", (10240, 3), 4, 13),
]  # fmt: skip


@functools.lru_cache(maxsize=None)
def band_end_case(path: str, shape: Tuple[int, int], w: int, width: int) -> Case:
    """The window that would start one channel after the band's last full window must not count.
    The last ``w - 1`` channels of every baseline are big samples (64 + 3 * 2**-24 each), the
    channel before them is amplitude 0 (deviation -m, about -1), and ``w * thr_k`` is
    ``64 (w - 1) - 0.5``: the last full window sums to about half a unit less than the limit and
    does not fire, while the ``w - 1`` samples alone -- a window padded with one zero beyond the
    band -- exceed it. Falloff 2.0 as elsewhere; no window of any size fires, nothing is flagged."""
    channels, baselines = shape
    n = w - 1
    amp = np.full(shape, M_EXACT, np.float32)
    amp[::5] = M_EXACT - Q
    amp[channels - 2 * w : channels - w] = M_EXACT
    amp[channels - w] = 0
    amp[channels - n :] = BIG
    target = np.float32((64.0 * n - 0.5) / w)
    k = w.bit_length() - 1
    noise = float(host.MAD_NORMAL) * 0.25
    n_sigma = _aim_sum(noise, pow(2.0, -k), target)
    vis = amp.astype(np.complex64)
    vis.setflags(write=False)
    case = Case(f"{path}_{channels}x{baselines}_band_end_w{w}", path, "sum", "exact", w, False, vis,
                False, width, n_sigma, 4, 2.0, False, None, [], target)  # fmt: skip
    dev, got_noise, exact, _ = case.host_stages()
    assert np.all(got_noise == noise), case.name
    thr = (n_sigma * got_noise * pow(2.0, -k)).astype(np.float32)
    assert np.all(thr == target), case.name
    limit = float(target) * w
    assert np.all(dev[channels - n :].sum(axis=0) > limit), case.name  # the padded window
    assert np.all(dev[channels - w :].sum(axis=0) < limit), case.name  # the last full one
    assert not exact.any(), case.name
    return case
