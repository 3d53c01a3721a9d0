"""NumPy restatement of the 2-D SumThreshold flagger (``rfi.twodflag``), stage by stage.

Test infrastructure, like ``rfi_oracle.c``: it imports only NumPy, conditions the
constructor's keywords itself and returns every temporary the HIP kernels keep, in the
workspace's ``[baseline][time][averaged channel]`` layout, so that a test can compare the
kernels with it stage by stage (``ksp_twodflag_layout``) at any shape. The arithmetic is
DESIGN.md section 9's: numba's typing of the reference, and every sum the reference carries
along a line (the four box passes, SumThreshold's cumulative sums) in that line's
sequential order. ``np.cumsum`` (``add.accumulate``) is sequential, so it is the only
summation used for those; the lines themselves are vectorised.
"""

import math

import numpy as np

MAD_NORMAL = 1.4826
#: lanes per block of the box filter (bounds the float64 temporaries)
_BOX_LANES = 2048

#: the reference constructor's keywords and defaults
DEFAULTS = {
    "outlier_nsigma": 4.5, "windows_time": [1, 2, 4, 8], "windows_freq": [1, 2, 4, 8],
    "background_reject": 2.0, "background_iterations": 1, "spike_width_time": 12.5,
    "spike_width_freq": 10.0, "time_extend": 3, "freq_extend": 3, "freq_chunks": 10,
    "average_freq": 1, "flag_all_time_frac": 0.6, "flag_all_freq_frac": 0.8, "rho": 1.3,
}  # fmt: skip

#: stage name -> (dtype, axes) in the workspace layout; B baselines, T times,
#: A averaged channels, F input channels
STAGES = {
    "spec_flags": (np.uint8, "BA"),  # median spectrum flags
    "spec_background": (np.float32, "BA"),
    "spec_residual": (np.float32, "BA"),  # median spectrum - its background
    "spec_st": (np.uint8, "BA"),  # SumThreshold flags of the spectrum
    "flags": (np.uint8, "BTA"),  # averaged flags | spectrum flags
    "background": (np.float32, "BTA"),
    "residual": (np.float32, "BTA"),  # averaged data - 2-D background
    "time_flags": (np.uint8, "BTA"),
    "freq_flags": (np.uint8, "BTA"),
    "combined": (np.uint8, "BTA"),  # spectrum | time | frequency, smeared in time
    "row_flags": (np.uint8, "BTF"),  # un-averaged and smeared in frequency
    "row_all": (np.uint8, "BT"),  # whole-time-row flags
    "col_all": (np.uint8, "BF"),  # whole-channel flags
}  # fmt: skip


class Config:
    """The reference's conditioning of its constructor keywords for one block shape."""

    def __init__(self, n_time, n_freq, **kw):
        unknown = set(kw) - set(DEFAULTS)
        if unknown:
            raise TypeError(f"unknown keywords {sorted(unknown)}")
        k = dict(DEFAULTS, **kw)
        average_freq = int(k["average_freq"])
        self.n_time, self.n_freq, self.average_freq = int(n_time), int(n_freq), average_freq
        self.n_avg = (self.n_freq + average_freq - 1) // average_freq
        # frequency windows: scaled (float32, as the constructor does) and made unique
        wf = np.ceil(np.asarray(k["windows_freq"], np.float32) / np.float32(average_freq))
        wf = np.unique(wf.astype(np.int64))
        # time windows: as given, duplicates and order kept, but clipped against the
        # number of CHANNELS (the reference's quirk)
        self.windows_time = [int(w) for w in k["windows_time"] if w <= self.n_freq]
        self.windows_freq = [int(w) for w in wf if w <= self.n_avg]
        if not self.windows_time or not self.windows_freq:
            raise ValueError("no window is left after clipping")
        rho = float(k["rho"])
        self.tf_time = [rho ** float(np.log2(w)) for w in self.windows_time]
        self.tf_freq = [rho ** float(np.log2(w)) for w in self.windows_freq]
        ends = np.linspace(0, self.n_avg, int(k["freq_chunks"]) + 1).astype(np.int64)
        self.chunks = [(int(a), int(b)) for a, b in zip(ends[:-1], ends[1:])]
        self.iterations = int(k["background_iterations"])
        self.spike_width_time = float(k["spike_width_time"])
        self.spike_width_freq = float(k["spike_width_freq"]) / average_freq
        self.time_extend, self.freq_extend = int(k["time_extend"]), int(k["freq_extend"])
        self.threshold_scale = float(k["outlier_nsigma"]) * MAD_NORMAL
        self.reject_scale = MAD_NORMAL * float(k["background_reject"])
        self.flag_all_time_frac = float(k["flag_all_time_frac"])
        self.flag_all_freq_frac = float(k["flag_all_freq_frac"])


def radius(sigma):
    """Box radius of the 4-pass Gaussian approximation for one axis's sigma."""
    return int(0.5 * math.sqrt(12.0 * (sigma * sigma) / 4 + 1))


def divisor(r):
    """numba's float32 ``d ** 4``: squared twice in float32."""
    a = np.float32(2 * r + 1) * np.float32(2 * r + 1)
    return np.float32(a * a)


# ------------------------------------------------------------------ medians
def _median_f64(values):
    """numba's ``np.median`` of a 1-D float32 array (size >= 1): float64."""
    n = values.size
    half = n // 2
    if n & 1:
        return float(np.partition(values, half)[half])
    part = np.partition(values, [half - 1, half])
    return float(np.float32(part[half - 1] + part[half])) / 2.0


def _median_lanes(x, valid):
    """Per lane (row) median of the valid float32 values, stored in float32 as the
    reference's float32 result arrays do; NaN for a lane without one."""
    n = x.shape[1]
    s = np.sort(np.where(valid, x, np.float32(np.nan)), axis=1)
    count = valid.sum(axis=1)
    half = count // 2
    hi = np.take_along_axis(s, np.minimum(half, n - 1)[:, None], axis=1)[:, 0]
    lo = np.take_along_axis(s, np.maximum(half - 1, 0)[:, None], axis=1)[:, 0]
    even = ((lo + hi).astype(np.float64) / 2.0).astype(np.float32)
    med = np.where(count % 2 == 1, hi, even)
    return np.where(count == 0, np.float32(np.nan), med).astype(np.float32), count


# ------------------------------------------------------------------ background
def _box_sums(lines, r):
    """The four box passes of one float32 line per row, padded by 4r zeros on the left:
    float64 running sums stored into the float32 line, in the reference's order. Each
    pass reads only the previous pass's values, so its running sum is one sequential
    cumsum of the interleaved terms (+new, -old, +new, ...)."""
    lanes, n = lines.shape
    pad, r2 = 4 * r, 2 * r
    L = n + pad
    P = np.zeros((lanes, L), np.float32)
    P[:, pad:] = lines
    prev_start = pad
    for p in range(1, 5):
        start = pad - r2 * p
        stop = start + n + 2 * pad
        start, stop = max(start, 0), min(stop, L)
        tail = min(stop, L - r2)
        head = P[:, prev_start:min(start + r2, L)]
        k0, na, nb = head.shape[1], tail - start, stop - tail
        assert na >= 1 and nb >= 0
        terms = np.empty((lanes, k0 + 2 * na + nb), np.float64)
        terms[:, :k0] = head
        terms[:, k0:k0 + 2 * na:2] = P[:, start + r2:tail + r2]
        terms[:, k0 + 1:k0 + 2 * na:2] = -P[:, start:tail]
        terms[:, k0 + 2 * na:] = -P[:, tail:stop]
        run = np.cumsum(terms, axis=1)
        P[:, start:tail] = run[:, k0:k0 + 2 * na:2]
        P[:, tail:stop] = run[:, k0 + 2 * na - 1:k0 + 2 * na - 1 + nb]
        prev_start = start
    return P[:, :n]


def _box_filter(lines, r):
    """Box filter of every row (r > 0), divided by numba's float32 d ** 4."""
    out = np.empty_like(lines)
    div = divisor(r)
    for i in range(0, lines.shape[0], _BOX_LANES):
        out[i:i + _BOX_LANES] = _box_sums(lines[i:i + _BOX_LANES], r) / div
    return out


def _smooth(img, rt, rf):
    """``_box_gaussian_filter`` of (B, T, A) images: along time, then along frequency."""
    B, T, A = img.shape
    if rt > 0:
        lines = np.ascontiguousarray(img.transpose(0, 2, 1)).reshape(B * A, T)
        img = _box_filter(lines, rt).reshape(B, A, T).transpose(0, 2, 1)
    if rf > 0:
        img = _box_filter(np.ascontiguousarray(img).reshape(B * T, A), rf).reshape(B, T, A)
    return np.ascontiguousarray(img, np.float32)


def _masked_filter(data, flags, rt, rf):
    weight = _smooth(np.where(flags, np.float32(0), np.float32(1)), rt, rf)
    out = _smooth(np.where(flags, np.float32(0), data), rt, rf)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(weight == 0, np.float32(np.nan), out / weight).astype(np.float32)


def _interpolate_nans(rows):
    """``_linearly_interpolate_nans1d`` of every row: ends repeated outwards, straight
    lines across interior gaps (gradient and values in float64), all-NaN rows zero."""
    lanes, n = rows.shape
    valid = ~np.isnan(rows)
    idx = np.broadcast_to(np.arange(n), rows.shape)
    left = np.maximum.accumulate(np.where(valid, idx, -1), axis=1)
    right = np.minimum.accumulate(np.where(valid, idx, n)[:, ::-1], axis=1)[:, ::-1]
    lv = np.take_along_axis(rows, np.maximum(left, 0), axis=1)
    rv = np.take_along_axis(rows, np.minimum(right, n - 1), axis=1)
    gap = np.maximum(right - left, 1).astype(np.float64)
    grad = (rv - lv).astype(np.float64) / gap
    inner = (lv.astype(np.float64) + (idx - left).astype(np.float64) * grad).astype(np.float32)
    out = np.where(left < 0, rv, np.where(right >= n, lv, inner))
    out = np.where(valid, rows, out)
    out[~valid.any(axis=1)] = 0
    return out.astype(np.float32)


def background(data, flags, cfg, sw_time, sw_freq):
    """``_get_background2d`` of (B, T, A) images: iterated masked smoothing with outlier
    rejection per frequency chunk, the final smoothing, NaNs interpolated along frequency."""
    B, T, A = data.shape
    work = flags.astype(np.bool_).copy()
    for ef in range(cfg.iterations, 0, -1):
        bg = _masked_filter(data, work, radius(ef * sw_time), radius(ef * sw_freq))
        res = np.abs(data - bg)
        for c0, c1 in cfg.chunks:
            if c1 <= c0:
                continue
            for b in range(B):
                sub = res[b, :, c0:c1]
                vals = sub[~work[b, :, c0:c1]]
                if vals.size == 0:
                    continue  # NaN threshold: nothing is flagged
                thr = _median_f64(vals) * cfg.reject_scale
                work[b, :, c0:c1] |= sub.astype(np.float64) > thr
    bg = _masked_filter(data, work, radius(sw_time), radius(sw_freq))
    return _interpolate_nans(bg.reshape(B * T, A)).reshape(B, T, A)


# ------------------------------------------------------------------ SumThreshold
def _smear(hits, w, P):
    """(lanes, P) flags: a position is hit when a window average starting in
    [i - w + 1, i] is; `hits` holds the m = P - w + 1 window starts."""
    m = hits.shape[1]
    if m <= 0:
        return np.zeros((hits.shape[0], P), np.bool_)
    run = np.zeros((hits.shape[0], m + 1), np.int64)
    run[:, 1:] = np.cumsum(hits, axis=1)
    i = np.arange(P)
    hi = np.minimum(i + 1, m)
    lo = np.clip(i - w + 1, 0, m)
    return run[:, hi] != run[:, lo]


def sum_threshold(x, flagged, chunks, windows, tfs, threshold_scale):
    """``_sum_threshold1d`` of every row of x (lanes, n) float32, with the row's chunks;
    returns the flags (lanes, n) bool."""
    lanes, n = x.shape
    out = np.zeros((lanes, n), np.bool_)
    maxw = max(windows)
    for c0, c1 in chunks:
        if c1 <= c0:
            continue
        med, count = _median_lanes(np.abs(x[:, c0:c1]), ~flagged[:, c0:c1])
        thr = (med.astype(np.float64) * threshold_scale).astype(np.float32)
        thr = np.where(count == 0, np.float32(np.inf), thr)
        p0, p1 = max(c0 - maxw + 1, 0), min(c1 + maxw - 1, n)
        P = p1 - p0
        seg = x[:, p0:p1].astype(np.float64)
        pos = np.zeros((lanes, P), np.bool_)
        neg = np.zeros((lanes, P), np.bool_)
        for w, tf in zip(windows, tfs):
            lim = (thr.astype(np.float64) / tf)[:, None]
            clamped = np.where(pos & (seg > lim), lim, np.where(neg & (seg < -lim), -lim, seg))
            terms = np.zeros((lanes, P + 1), np.float64)
            terms[:, 1:] = clamped
            cum = np.cumsum(terms, axis=1)  # cum[0] = 0 + nothing; cum[i + 1] = cum[i] + v
            cum[:, 0] = 0.0
            m = P + 1 - w
            avg = cum[:, w:] - cum[:, :m] if m > 0 else np.zeros((lanes, 0))
            scale = np.float32(1.0 / w)
            pos |= _smear(avg * np.float64(scale) > lim, w, P)
            neg |= _smear(avg * np.float64(-scale) > lim, w, P)
        out[:, c0:c1] = (pos | neg)[:, c0 - p0:c1 - p0]
    return out


# ------------------------------------------------------------------ whole flagger
def _average(data, in_flags, factor):
    """|z| (or |x|), NaN and flagged samples left out, frequency groups added in channel
    order in float32 and divided by their count. (B, T, A) data and flags."""
    T, F, B = data.shape
    A = (F + factor - 1) // factor
    amp = np.abs(data).astype(np.float32)
    valid = (in_flags == 0) & ~np.isnan(amp)
    total = np.zeros((T, A, B), np.float32)
    weight = np.zeros((T, A, B), np.int64)
    for k in range(min(factor, F)):
        ch = np.arange(k, F, factor)
        total[:, ch // factor] += np.where(valid[:, ch], amp[:, ch], np.float32(0))
        weight[:, ch // factor] += valid[:, ch]
    empty = weight == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        avg = np.where(empty, np.float32(0), total / weight.astype(np.float32))
    return (np.ascontiguousarray(avg.transpose(2, 0, 1), np.float32),
            np.ascontiguousarray(empty.transpose(2, 0, 1)))  # fmt: skip


def _window_counts(flags, extend, axis_len):
    """Box smearing by `extend` along the last axis: any flag in [i + lo, i + hi)."""
    lo = -(extend // 2)
    hi = lo + extend
    run = np.zeros(flags.shape[:-1] + (axis_len + 1,), np.int64)
    run[..., 1:] = np.cumsum(flags, axis=-1)
    i = np.arange(axis_len)
    return run[..., np.minimum(i + hi, axis_len)] != run[..., np.maximum(i + lo, 0)]


def flag(data, in_flags, **kw):
    """Flags of the reference's ``SumThresholdFlagger(**kw).get_flags(data, in_flags)`` and
    every stage: returns (flags (time, channel, baseline) bool, {stage: array})."""
    if data.ndim != 3 or data.shape != in_flags.shape:
        raise ValueError("data and flags must be (time, channel, baseline) of one shape")
    if data.dtype not in (np.complex64, np.float32):
        raise TypeError("data must be complex64 or float32")
    T, F, B = data.shape
    cfg = Config(T, F, **kw)
    A = cfg.n_avg
    avg, flg = _average(data, in_flags, cfg.average_freq)

    # median spectrum, its background and SumThreshold
    med, count = _median_lanes(avg.transpose(0, 2, 1).reshape(B * A, T),
                               ~flg.transpose(0, 2, 1).reshape(B * A, T))  # fmt: skip
    spec_flags = (count == 0).reshape(B, A)
    spec = np.where(spec_flags, np.float32(0), med.reshape(B, A)).astype(np.float32)
    spec_bg = background(spec[:, None], spec_flags[:, None], cfg, 0.0, cfg.spike_width_freq)[:, 0]
    spec_res = spec - spec_bg
    spec_st = sum_threshold(spec_res, spec_flags, cfg.chunks, cfg.windows_freq, cfg.tf_freq,
                            cfg.threshold_scale)  # fmt: skip

    # 2-D background, SumThreshold along time, then along frequency with the time flags
    flags2 = flg | spec_st[:, None, :]
    bg = background(avg, flags2, cfg, cfg.spike_width_time, cfg.spike_width_freq)
    res = avg - bg
    res_t = np.ascontiguousarray(res.transpose(0, 2, 1)).reshape(B * A, T)
    fl_t = np.ascontiguousarray(flags2.transpose(0, 2, 1)).reshape(B * A, T)
    tfl = sum_threshold(res_t, fl_t, [(0, T)], cfg.windows_time, cfg.tf_time,
                        cfg.threshold_scale).reshape(B, A, T).transpose(0, 2, 1)  # fmt: skip
    ffl = sum_threshold(res.reshape(B * T, A), (flags2 | tfl).reshape(B * T, A), cfg.chunks,
                        cfg.windows_freq, cfg.tf_freq, cfg.threshold_scale).reshape(B, T, A)

    # combined flags smeared in time; un-averaged, smeared in frequency; whole rows/columns
    comb = spec_st[:, None, :] | tfl | ffl
    comb = _window_counts(comb.transpose(0, 2, 1), cfg.time_extend, T).transpose(0, 2, 1)
    rep = comb[:, :, np.arange(F) // cfg.average_freq]
    rows = _window_counts(rep, cfg.freq_extend, F)
    row_all = rows.sum(axis=2).astype(np.float64) > cfg.flag_all_freq_frac * F
    col_all = rows.sum(axis=1).astype(np.float64) > float(T) * cfg.flag_all_time_frac
    out = rows | row_all[:, :, None] | col_all[:, None, :]
    out = out.transpose(1, 2, 0) | np.isnan(data)

    stages = {
        "spec_flags": spec_flags, "spec_background": spec_bg, "spec_residual": spec_res,
        "spec_st": spec_st, "flags": flags2, "background": bg, "residual": res,
        "time_flags": tfl, "freq_flags": ffl, "combined": comb, "row_flags": rows,
        "row_all": row_all, "col_all": col_all,
    }  # fmt: skip
    stages = {k: np.ascontiguousarray(v, STAGES[k][0]) for k, v in stages.items()}
    return np.ascontiguousarray(out), stages
