"""Host-side (NumPy) interface of the RFI flaggers.

The abstract classes are the call signatures that the ``*HostFromDevice`` adapters in
:mod:`katsdpsigproc_amd.rfi.device` present, and the concrete classes give the package
the same host API as the reference (reference: src/katsdpsigproc/rfi/host.py:28-273).
They are whole-array NumPy formulations (no pandas, no per-baseline Python loops) with
the same numerics, dtype for dtype, as the reference classes; ``tests/test_host.py``
checks them against golden vectors produced by the reference.

Nothing in the device path calls this module: device operations run HIP kernels only
and raise if the native library is missing.
"""

import warnings
from abc import ABC, abstractmethod
from typing import Optional, Tuple

import numpy as np

from . import MAD_NORMAL, BackgroundFlags


class AbstractBackgroundHost(ABC):
    @abstractmethod
    def __init__(self, width: int, amplitudes: bool = False) -> None: ...

    @abstractmethod
    def __call__(self, vis: np.ndarray, flags: Optional[np.ndarray] = None) -> np.ndarray:
        """Deviation of each amplitude from a smooth background.

        `vis` is channels x baselines (complex, or amplitudes if constructed with
        ``amplitudes=True``); `flags` (optional, per channel or full shape) marks samples
        that must not influence the background. Returns float deviations, 0 where
        flagged.
        """


class AbstractNoiseEstHost(ABC):
    @abstractmethod
    def __call__(self, deviations: np.ndarray) -> np.ndarray:
        """Per-baseline noise (standard deviation) estimate from channels x baselines deviations."""


class AbstractThresholdHost(ABC):
    @abstractmethod
    def __init__(self, n_sigma: float) -> None: ...

    @abstractmethod
    def __call__(self, deviations: np.ndarray, noise: np.ndarray) -> np.ndarray:
        """uint8 flags (flag value or 0) with the shape of `deviations`."""


class AbstractFlaggerHost(ABC):
    @abstractmethod
    def __call__(self, vis: np.ndarray, input_flags: Optional[np.ndarray] = None) -> np.ndarray:
        """uint8 flags for channels x baselines visibilities.

        `input_flags` only steer the background; they are not copied to the output and a
        sample flagged on input is never flagged on output.
        """


class BackgroundMedianFilterHost(AbstractBackgroundHost):
    """Amplitude minus its centred sliding median along channels.

    The window is clipped at the band edges and skips flagged, NaN and infinite samples
    (pandas turns +-inf into NaN before its rolling median); an even number of valid
    samples gives the mean of the middle two. The deviation is taken from the unmasked
    amplitude, so an infinite sample keeps ``inf - median``, and ``inf - NaN`` (no finite
    sample in the window) becomes 0 like every other NaN. Amplitudes are float32, the
    median and the result float64 (as the reference, rfi/host.py:133-151).
    """

    #: baselines processed per block, to bound the size of the window tensor
    _BLOCK = 256

    def __init__(self, width: int, amplitudes: bool = False) -> None:
        if width % 2 != 1:
            raise ValueError("width must be odd")
        self.width = width
        self.amplitudes = amplitudes

    def __call__(self, vis: np.ndarray, flags: Optional[np.ndarray] = None) -> np.ndarray:
        vis = np.asarray(vis)
        amp = vis if self.amplitudes else np.abs(vis)
        amp = amp.astype(np.float64)  # exact; the median is taken in float64
        channels, baselines = amp.shape
        if flags is not None:
            mask = np.asarray(flags).astype(np.bool_)
            if mask.ndim == 1:
                mask = mask[:, np.newaxis]
            amp = np.where(np.broadcast_to(mask, amp.shape), np.nan, amp)
        win_amp = np.where(np.isinf(amp), np.nan, amp)  # what the rolling median sees
        half = self.width // 2
        out = np.empty((channels, baselines), np.float64)
        pad = np.full((half, 1), np.nan)
        for start in range(0, baselines, self._BLOCK):
            block = win_amp[:, start : start + self._BLOCK]
            padded = np.concatenate(
                [np.broadcast_to(pad, (half, block.shape[1])), block,
                 np.broadcast_to(pad, (half, block.shape[1]))]
            )  # fmt: skip
            windows = np.lib.stride_tricks.sliding_window_view(padded, self.width, axis=0)
            ordered = np.sort(windows, axis=-1)  # NaN sorts last
            count = np.sum(~np.isnan(windows), axis=-1)
            lo = np.take_along_axis(ordered, np.maximum(count - 1, 0)[..., None] // 2, -1)[..., 0]
            hi = np.take_along_axis(ordered, (count // 2)[..., None], -1)[..., 0]
            median = (lo + hi) / 2.0
            with np.errstate(invalid="ignore"):
                dev = amp[:, start : start + self._BLOCK] - median
            out[:, start : start + self._BLOCK] = np.where(np.isnan(dev), 0.0, dev)
        return out


class NoiseEstMADHost(AbstractNoiseEstHost):
    """``1.4826 * median(|d| : d != 0)`` per baseline.

    The median keeps the dtype of `deviations` (float32 in, float32 median -- even counts
    average in float32, odd counts take the middle value itself), the scale is applied in
    float64 (reference rfi/host.py:157-163). A baseline with no non-zero deviation gives
    NaN.
    """

    def __call__(self, deviations: np.ndarray) -> np.ndarray:
        mag = np.abs(np.asarray(deviations))
        ordered = np.sort(np.where(mag > 0, mag, np.inf), axis=0)  # zeros pushed to the end
        count = np.sum(mag > 0, axis=0)
        cols = np.arange(mag.shape[1])
        lo = ordered[np.maximum(count - 1, 0) // 2, cols]
        hi = ordered[np.minimum(count // 2, mag.shape[0] - 1), cols]
        with np.errstate(invalid="ignore", over="ignore"):
            median = np.where(count % 2 == 1, lo, (lo + hi) / mag.dtype.type(2))
        median = np.where(count > 0, median, np.nan)
        if np.any(count == 0):
            warnings.warn("baseline with no non-zero deviations", RuntimeWarning)
        return median.astype(np.float64) * MAD_NORMAL


class ThresholdSimpleHost(AbstractThresholdHost):
    """Flag samples whose deviation exceeds ``n_sigma * noise`` of their baseline."""

    def __init__(self, n_sigma: float, flag_value: int = 1) -> None:
        self.n_sigma = n_sigma
        self.flag_value = flag_value

    def __call__(self, deviations: np.ndarray, noise: np.ndarray) -> np.ndarray:
        limit = self.n_sigma * np.asarray(noise)  # keeps noise's dtype (NEP 50)
        return (np.asarray(deviations) > limit).astype(np.uint8) * np.uint8(self.flag_value)


class ThresholdSumHost(AbstractThresholdHost):
    """Offringa SumThreshold along channels with windows 1, 2, 4, ... (rfi/host.py:186-254).

    For window ``w = 2**k`` the per-sample threshold is
    ``float32(n_sigma * noise * falloff**-k)``; samples flagged by earlier windows are
    replaced by that threshold; every full window whose float64 sum exceeds
    ``float32(threshold * w)`` flags all its samples. All baselines are processed
    together.
    """

    def __init__(self, n_sigma: float, n_windows: int = 4, threshold_falloff: float = 1.2,
                 flag_value: int = 1) -> None:  # fmt: skip
        self.n_sigma = n_sigma
        self.windows = [2**i for i in range(n_windows)]
        self.threshold_scales = [pow(threshold_falloff, -i) for i in range(n_windows)]
        self.flag_value = flag_value

    def __call__(self, deviations: np.ndarray, noise: np.ndarray) -> np.ndarray:
        work = np.array(deviations, dtype=np.float64)  # exact copy of float32 input
        channels = work.shape[0]
        threshold1 = self.n_sigma * np.asarray(noise)  # float32 stays float32
        flagged = np.zeros(work.shape, np.bool_)
        for window, scale in zip(self.windows, self.threshold_scales):
            threshold = (threshold1 * scale).astype(np.float32)
            work = np.where(flagged, threshold[np.newaxis, :], work)
            n_sums = channels - window + 1
            if n_sums <= 0:
                continue
            sums = work[:n_sums].copy()
            for offset in range(1, window):  # same left-to-right order as numpy.convolve
                sums += work[offset : offset + n_sums]
            with np.errstate(invalid="ignore"):
                hit = sums > (threshold * np.float32(window))[np.newaxis, :]
            for offset in range(window):
                flagged[offset : offset + n_sums] |= hit
        return flagged.astype(np.uint8) * np.uint8(self.flag_value)


def check_flag_masks(masks) -> tuple:
    """`masks` of a flag counter as a tuple of ints: 1 to 8 values, each 1..255
    (``ValueError`` otherwise, ``TypeError`` for a value that is not an integer)."""
    masks = tuple(masks)
    for mask in masks:
        if isinstance(mask, (bool, np.bool_)) or not isinstance(mask, (int, np.integer)):
            raise TypeError(f"mask {mask!r} is not an integer")
    if not 1 <= len(masks) <= 8:
        raise ValueError("masks must hold between 1 and 8 values")
    for mask in masks:
        if not 1 <= mask <= 255:
            raise ValueError(f"mask {mask} is outside 1..255")
    return tuple(int(mask) for mask in masks)


class FlagCountHost:
    """How many samples are flagged, per channel and per baseline.

    For every mask ``m`` of `masks` (1 to 8 integers in 1..255; the default counts any
    flag), ``channel_counts[m][c]`` is the number of baselines whose flag byte at channel
    ``c`` has a bit of the mask set, ``baseline_counts[m][b]`` the number of such channels of
    baseline ``b``. A sample counts at most once per mask; masks may overlap. No reference
    counterpart.
    """

    def __init__(self, masks=(0xFF,)) -> None:
        self.masks = check_flag_masks(masks)

    def __call__(self, flags: np.ndarray):
        """(channel_counts, baseline_counts), both uint32, ``len(masks)`` rows, for channels x
        baselines uint8 `flags`."""
        flags = np.asarray(flags)
        if flags.ndim != 2 or flags.dtype != np.uint8:
            raise ValueError("flags must be a 2-D uint8 array")
        channel_counts = np.empty((len(self.masks), flags.shape[0]), np.uint32)
        baseline_counts = np.empty((len(self.masks), flags.shape[1]), np.uint32)
        for i, mask in enumerate(self.masks):
            hit = (flags & np.uint8(mask)) != 0
            channel_counts[i] = np.count_nonzero(hit, axis=1)
            baseline_counts[i] = np.count_nonzero(hit, axis=0)
        return channel_counts, baseline_counts


def check_flag_byte(name: str, value) -> int:
    """`value` as an int in 1..255 (``ValueError`` otherwise, ``TypeError`` for a value that
    is not an integer), as :func:`check_flag_masks` checks a mask."""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
        raise TypeError(f"{name} {value!r} is not an integer")
    if not 1 <= value <= 255:
        raise ValueError(f"{name} {value} is outside 1..255")
    return int(value)


class ScaleInvariantRankHost:
    """Scale-invariant rank (SIR) operator along the channel axis: extends the flags of
    every baseline over the gaps between them (Offringa, van de Gronde & Roerdink 2012).

    A sample counts as flagged when ``flags & mask != 0``. Every sample of every channel
    interval ``[a, b)`` of a baseline with

        ``4096 * #flagged(a, b) >= (4096 - eta_q) * (b - a)``

    is in the result and gets ``flags |= flag_value``; every other bit of every byte is kept.
    ``eta_q = floor(eta * 4096 + 0.5)`` quantises `eta` once, so that all arithmetic is
    integer and the device operation (:class:`.device.ScaleInvariantRankTemplate`) matches
    this class bit for bit. The result contains the input; ``eta = 0`` adds nothing,
    ``eta = 1`` flags every sample, those of a baseline without any flag included. No
    reference counterpart.

    The implementation is the running-sum form of the rule: with ``psi = eta_q`` for a
    flagged sample and ``eta_q - 4096`` for any other, and ``M(j)`` the sum of ``psi`` over the
    channels below ``j``, channel ``x`` is in the result iff the largest ``M(b)``,
    ``x < b <= channels``, is at least the smallest ``M(a)``, ``0 <= a <= x``.

    Parameters
    ----------
    eta
        Aggressiveness in [0, 1] (``ValueError`` outside it or for NaN): an interval is
        flagged when at most that share of it, quantised, is unflagged
    mask
        Which bits make a sample count as flagged, 1..255 (``ValueError`` outside,
        ``TypeError`` for a non-integer); default any
    flag_value
        Bits set in every sample of the result, 1..255 (as `mask`); may overlap `mask`
    """

    def __init__(self, eta: float, mask: int = 0xFF, flag_value: int = 1) -> None:
        eta = float(eta)
        if not 0.0 <= eta <= 1.0:  # (NaN fails both comparisons)
            raise ValueError(f"eta {eta} is outside [0, 1]")
        self.eta = eta
        self.eta_q = int(np.floor(eta * 4096.0 + 0.5))
        self.mask = check_flag_byte("mask", mask)
        self.flag_value = check_flag_byte("flag_value", flag_value)

    def __call__(self, flags: np.ndarray) -> np.ndarray:
        """A new channels x baselines uint8 array: `flags` with the result ORed in."""
        flags = np.asarray(flags)
        if flags.ndim != 2 or flags.dtype != np.uint8:
            raise ValueError("flags must be a 2-D uint8 array")
        flagged = (flags & np.uint8(self.mask)) != 0
        psi = np.where(flagged, np.int64(self.eta_q), np.int64(self.eta_q - 4096))
        m = np.zeros((flags.shape[0] + 1, flags.shape[1]), np.int64)
        np.cumsum(psi, axis=0, out=m[1:])
        lowest = np.minimum.accumulate(m[:-1], axis=0)  # over a in [0, x]
        highest = np.maximum.accumulate(m[:0:-1], axis=0)[::-1]  # over b in (x, channels]
        return flags | np.where(highest >= lowest, np.uint8(self.flag_value), np.uint8(0))


class AveragerHost:
    """Flag-aware averaging of visibilities over dumps and over groups of channels.

    :meth:`add` accumulates one dump into ``acc_vis`` (complex64), ``acc_weights`` (float32)
    and ``acc_flags`` (uint8), all channels x baselines; :meth:`finalise` sums every
    `channel_factor` adjacent channels, divides by the weight, returns
    ``(vis, weights, flags)`` of ``channels // channel_factor`` rows and clears the state.
    No reference counterpart; this class is the definition that the device operations
    (:class:`.device.AccumulateTemplate`, :class:`.device.FinaliseTemplate`) match bit for
    bit.

    A flagged sample is not dropped but enters with its weight scaled by 2**-64. An output
    with at least one unflagged contribution is then, to rounding, the weighted average of
    the unflagged ones; an output whose contributions were all flagged carries the average
    of the flagged data (its sums are scaled back by 2**64) and the OR of their flags.
    One set of accumulators serves both cases.

    Every step is one float32 operation, rounded once, in the order written in the methods
    (a multiply and then an add, never a fused multiply-add; two real divisions, not a
    complex one). NaN, infinity and denormals go through as IEEE arithmetic gives them.

    The caller's side of the contract: a weight is 0 ("no data") or within about
    [2**-30, 2**30], and an output sums at most about 2**30 contributions, so that the
    threshold 2**-32 on the summed weight tells "some unflagged data" from "flagged data
    only". An output with no data at all has weight 0, visibility 0 and flags 0.

    Parameters
    ----------
    channels, baselines
        Shape of a dump (``ValueError`` if below 1)
    channel_factor
        Number of adjacent channels per output channel (``ValueError`` unless it is at
        least 1 and divides `channels`)
    input_flags
        :class:`BackgroundFlags` (or its value): whether :meth:`add` also takes a static
        mask, per channel (CHANNEL) or per sample (FULL), that is ORed into the flags
    """

    FLAGGED_SCALE = np.float32(2.0 ** -64)
    UNSCALE = np.float32(2.0 ** 64)
    ALL_FLAGGED_BELOW = np.float32(2.0 ** -32)

    def __init__(self, channels: int, baselines: int, channel_factor: int = 1,
                 input_flags=BackgroundFlags.NONE) -> None:  # fmt: skip
        if channels < 1 or baselines < 1:
            raise ValueError("channels and baselines must be at least 1")
        if channel_factor < 1 or channels % channel_factor:
            raise ValueError("channel_factor must be at least 1 and divide channels")
        self.channels = channels
        self.baselines = baselines
        self.channel_factor = channel_factor
        self.input_flags = BackgroundFlags(input_flags)
        self.acc_vis = np.zeros((channels, baselines), np.complex64)
        self.acc_weights = np.zeros((channels, baselines), np.float32)
        self.acc_flags = np.zeros((channels, baselines), np.uint8)

    def add(self, vis: np.ndarray, flags: np.ndarray, weights: Optional[np.ndarray] = None,
            input_flags: Optional[np.ndarray] = None) -> None:  # fmt: skip
        """Accumulate one dump: complex64 `vis`, uint8 `flags` (non-zero = flagged) and
        float32 `weights` (``None``: 1 everywhere), all channels x baselines, and uint8
        `input_flags` of shape (channels,) or (channels, baselines) as the mode says
        (``TypeError`` if given with mode NONE or missing otherwise)."""
        if input_flags is not None and not self.input_flags:
            raise TypeError("input_flags were provided but the mode is NONE")
        if input_flags is None and self.input_flags:
            raise TypeError("input_flags were expected but not provided")
        shape = (self.channels, self.baselines)
        vis = np.asarray(vis, np.complex64)
        f = np.asarray(flags, np.uint8)
        if vis.shape != shape or f.shape != shape:
            raise ValueError("vis and flags must be channels x baselines")
        if input_flags is not None:
            mask = np.asarray(input_flags, np.uint8)
            if self.input_flags == BackgroundFlags.CHANNEL:
                if mask.shape != (self.channels,):
                    raise ValueError("input_flags must have one byte per channel")
                mask = mask[:, np.newaxis]
            elif mask.shape != shape:
                raise ValueError("input_flags must be channels x baselines")
            f = f | mask
        if weights is None:
            w = np.ones(shape, np.float32)
        else:
            w = np.asarray(weights, np.float32)
            if w.shape != shape:
                raise ValueError("weights must be channels x baselines")
        bad = f != 0
        with np.errstate(all="ignore"):
            we = np.where(bad, w * self.FLAGGED_SCALE, w)
            self.acc_vis.real[...] = self.acc_vis.real + we * vis.real
            self.acc_vis.imag[...] = self.acc_vis.imag + we * vis.imag
            self.acc_weights[...] = self.acc_weights + we
        self.acc_flags |= f  # (f is zero wherever the sample is not flagged)

    def finalise(self):
        """``(vis, weights, flags)`` of ``channels // channel_factor`` x baselines from what
        has been accumulated; the state is zero again afterwards."""
        rows = self.channels // self.channel_factor
        grouped = (rows, self.channel_factor, self.baselines)
        acc_re = self.acc_vis.real.reshape(grouped)
        acc_im = self.acc_vis.imag.reshape(grouped)
        acc_w = self.acc_weights.reshape(grouped)
        acc_fl = self.acc_flags.reshape(grouped)
        re = np.zeros((rows, self.baselines), np.float32)
        im = np.zeros((rows, self.baselines), np.float32)
        w = np.zeros((rows, self.baselines), np.float32)
        fl = np.zeros((rows, self.baselines), np.uint8)
        with np.errstate(all="ignore"):
            for k in range(self.channel_factor):
                re = re + acc_re[:, k]
                im = im + acc_im[:, k]
                w = w + acc_w[:, k]
                fl = fl | acc_fl[:, k]
            allbad = w < self.ALL_FLAGGED_BELOW
            w = np.where(allbad, w * self.UNSCALE, w)
            re = np.where(allbad, re * self.UNSCALE, re)
            im = np.where(allbad, im * self.UNSCALE, im)
            some = w > 0
            vis = np.zeros((rows, self.baselines), np.complex64)
            vis.real[...] = np.where(some, re / w, np.float32(0))
            vis.imag[...] = np.where(some, im / w, np.float32(0))
        out_flags = np.where(allbad, fl, np.uint8(0))
        self.acc_vis[...] = 0
        self.acc_weights[...] = 0
        self.acc_flags[...] = 0
        return vis, w, out_flags


def _check_positive_float32(name: str, value) -> np.float32:
    """`value` as a finite, positive float32 (``ValueError`` otherwise)."""
    with np.errstate(all="ignore"):
        value32 = np.float32(value)
    if not (np.isfinite(value32) and value32 > 0):
        raise ValueError(f"{name} {value!r} is not a finite positive float32")
    return value32


def _check_array(name: str, value, dtype, shape_text: str, ok) -> np.ndarray:
    """`value` as an array, ``ValueError`` naming it unless it has `dtype` and `ok(shape)`."""
    value = np.asarray(value)
    if value.dtype != np.dtype(dtype) or not ok(value.shape):
        raise ValueError(f"{name} must be {np.dtype(dtype).name} of shape {shape_text}, not "
                         f"{value.dtype.name} {value.shape}")  # fmt: skip
    return value


class PrepareHost:
    """A correlator's integer dump as the inputs of the flagging chain: ``vis`` (complex64),
    ``input_flags`` (uint8, the FULL mask of the flagger and of :class:`AveragerHost`) and,
    optionally, ``weights`` (float32), all channels x baselines. No reference counterpart;
    this class is the definition that the device operation (:class:`.ingest.PrepareTemplate`)
    matches bit for bit.

    `vis_in` holds saturating int32 accumulations as (re, im) pairs in the correlator's own
    baseline order; ``source[j]`` names the input baseline that feeds output baseline ``j`` (a
    gather: repeats are allowed). A sample whose real part is ``-2**31`` was never received
    (a saturated accumulator clamps to ``+-(2**31 - 1)`` and never gives that value; an
    imaginary part of ``-2**31`` alone is data). Per channel ``c`` and output baseline ``j``::

        s    = source[j];  valid = 0 <= s < in_baselines
        lost = not valid or vis_in[c, s].re == -2**31
        vis  = lost ? 0 : (float32(re) * scale, float32(im) * scale)
        input_flags = cf | baseline_flags[j] | (lost ? lost_flag : 0)

    where ``cf`` is ``channel_flags[c]``, one static byte per channel for every baseline
    alike, or, with `mask_index`, the byte of the baseline's class of static mask (a known-RFI
    mask that applies to short baselines only, say)::

        k  = mask_index[j]                                  (uint8; any value is allowed)
        cf = k < classes ? channel_flags[k, c] : 0          (classes = len(channel_flags))

    An index of ``classes`` or more (255, say) means "no static mask for this baseline".
    ``baseline_flags[j]`` is ORed into every sample of baseline ``j`` (an antenna that is off
    target flags every baseline it takes part in); ``vis`` and ``weights`` do not depend on
    it, so :class:`AveragerHost` treats such a sample like any flagged one.

    And, with `auto_source` (the input baselines of the autocorrelations of the two inputs of
    every output baseline)::

        power(k) = valid k and vis_in[c, k].re != -2**31 ? float32(vis_in[c, k].re) * scale : 0
        pa, pb = power(auto_source[j, 0]), power(auto_source[j, 1]);  d = pa * pb
        weights = (pa > 0 and pb > 0 and d > 0) ? weight_scale / d : 0

    Every float step is one float32 operation, rounded once (the conversion from int32
    rounds to nearest even). A weight does not depend on whether its own sample is lost. Any
    int32 is allowed in `source` and `auto_source`; no NaN can arise.

    Parameters
    ----------
    scale, weight_scale
        Taken as ``np.float32``; finite and positive (``ValueError``)
    lost_flag
        Bits set in ``input_flags`` of a lost sample, 1..255 (:func:`check_flag_byte`)
    """

    LOST = np.int32(-(2**31))
    MAX_CLASSES = 8

    def __init__(self, scale: float = 1.0, lost_flag: int = 8, weight_scale: float = 1.0) -> None:
        self.scale = _check_positive_float32("scale", scale)
        self.lost_flag = check_flag_byte("lost_flag", lost_flag)
        self.weight_scale = _check_positive_float32("weight_scale", weight_scale)

    def _power(self, vis_in: np.ndarray, index: np.ndarray) -> np.ndarray:
        valid = (index >= 0) & (index < vis_in.shape[1])
        re = vis_in[:, np.where(valid, index, 0), 0]
        good = valid[np.newaxis, :] & (re != self.LOST)
        return np.where(good, re.astype(np.float32) * self.scale, np.float32(0))

    def __call__(self, vis_in: np.ndarray, source: np.ndarray,
                 channel_flags: Optional[np.ndarray] = None,
                 auto_source: Optional[np.ndarray] = None,
                 baseline_flags: Optional[np.ndarray] = None,
                 mask_index: Optional[np.ndarray] = None):  # fmt: skip
        """``(vis, input_flags, weights)`` for int32 `vis_in` (channels, in_baselines, 2),
        int32 `source` (baselines,), optional uint8 `channel_flags` (channels,), optional
        int32 `auto_source` (baselines, 2), optional uint8 `baseline_flags` (baselines,) and
        optional uint8 `mask_index` (baselines,), with which `channel_flags` is (classes,
        channels), classes 1..:attr:`MAX_CLASSES`, and without which it is not; ``weights`` is
        ``None`` without `auto_source`. ``ValueError``, naming the argument, for a wrong dtype,
        rank or shape."""
        vis_in = _check_array("vis_in", vis_in, np.int32, "(channels, in_baselines, 2)",
                              lambda s: len(s) == 3 and s[0] >= 1 and s[1] >= 1 and s[2] == 2)  # fmt: skip
        channels = vis_in.shape[0]
        source = _check_array("source", source, np.int32, "(baselines,)",
                              lambda s: len(s) == 1 and s[0] >= 1)  # fmt: skip
        baselines = source.shape[0]
        if mask_index is not None:
            mask_index = _check_array("mask_index", mask_index, np.uint8, "(baselines,)",
                                      lambda s: s == (baselines,))  # fmt: skip
            if channel_flags is None:
                raise ValueError("mask_index needs channel_flags of shape (classes, channels)")
            channel_flags = _check_array(
                "channel_flags", channel_flags, np.uint8,
                f"(classes, channels) with 1 to {self.MAX_CLASSES} classes",
                lambda s: len(s) == 2 and 1 <= s[0] <= self.MAX_CLASSES and s[1] == channels)
        elif channel_flags is not None:
            channel_flags = _check_array("channel_flags", channel_flags, np.uint8, "(channels,)",
                                         lambda s: s == (channels,))  # fmt: skip
        if auto_source is not None:
            auto_source = _check_array("auto_source", auto_source, np.int32, "(baselines, 2)",
                                       lambda s: s == (baselines, 2))  # fmt: skip
        if baseline_flags is not None:
            baseline_flags = _check_array("baseline_flags", baseline_flags, np.uint8,
                                          "(baselines,)", lambda s: s == (baselines,))  # fmt: skip
        valid = (source >= 0) & (source < vis_in.shape[1])
        picked = vis_in[:, np.where(valid, source, 0)]
        lost = ~valid[np.newaxis, :] | (picked[..., 0] == self.LOST)
        vis = np.zeros((channels, baselines), np.complex64)
        with np.errstate(all="ignore"):
            scaled = picked.astype(np.float32) * self.scale
        vis.real[...] = np.where(lost, np.float32(0), scaled[..., 0])
        vis.imag[...] = np.where(lost, np.float32(0), scaled[..., 1])
        input_flags = np.where(lost, np.uint8(self.lost_flag), np.uint8(0))
        if mask_index is not None:
            known = mask_index < channel_flags.shape[0]
            static = channel_flags[np.where(known, mask_index, 0)].T
            input_flags = input_flags | np.where(known[np.newaxis, :], static, np.uint8(0))
        elif channel_flags is not None:
            input_flags = input_flags | channel_flags[:, np.newaxis]
        if baseline_flags is not None:
            input_flags = input_flags | baseline_flags[np.newaxis, :]
        weights = None
        if auto_source is not None:
            with np.errstate(all="ignore"):
                pa = self._power(vis_in, auto_source[:, 0])
                pb = self._power(vis_in, auto_source[:, 1])
                d = pa * pb
                ok = (pa > 0) & (pb > 0) & (d > 0)
                # (the divisor of a sample that gets no weight is 1, not d: no 1 / 0)
                weights = np.where(ok, self.weight_scale / np.where(ok, d, np.float32(1)),
                                   np.float32(0))  # fmt: skip
            weights = np.ascontiguousarray(weights)  # (the gathers above come column-major)
        return vis, input_flags, weights


class CompressWeightsHost:
    """Float32 weights as one byte per sample and one float32 per channel: what a pipeline
    sends on instead of 4 bytes per sample. No reference counterpart; this class is the
    definition that the device operation (:class:`.ingest.CompressWeightsTemplate`) matches
    bit for bit. For row ``c``, every float step one float32 operation, rounded once::

        ok(w) = w > 0 and w < +inf
        m     = max over b of (ok(w[c, b]) ? w[c, b] : +0.0)       (+0.0 if no element is ok)
        wc    = m / 255                                  -> weights_channel[c]
        t     = w[c, b] / wc                             (IEEE, also when wc == 0)
        q     = not (w[c, b] > 0) ? 0 : (t >= 255 ? 255 : max(1, rint(t)))   -> weights8[c, b]

    (``rint`` rounds ties to even.) What follows from it:

    * The byte is 0 exactly where the weight is not positive: zero, -0.0, negative or NaN,
      which keeps :class:`AveragerHost`'s convention that weight 0 means "no data". A positive
      weight never becomes 0: that is what the ``max(1, ...)`` is for.
    * ``+inf`` takes no part in the maximum and becomes 255.
    * There is no special case for ``wc == 0``, which happens when no element is ok or when
      ``m / 255`` underflows to zero: ``w / 0`` is ``+inf``, so every positive weight becomes
      255, and ``255 * wc`` is 0. No NaN can arise in ``t`` for ``w > 0``.
    * When ``wc`` is a normal number (``m >= 2**-118``) the row's maximum maps to 255, and for
      every finite positive ``w`` of the row ``|q * wc - w| <= wc / 2`` to within rounding
      when ``q > 1`` and ``|q * wc - w| <= wc`` when ``q == 1``.
    * With a denormal ``wc`` the quotient ``m / wc`` ranges from 128 to 382; the result is
      then simply what the formula gives.
    """

    def __call__(self, weights: np.ndarray):
        """``(weights8, weights_channel)``: uint8 (channels, baselines) and float32
        (channels,) for float32 `weights` (channels, baselines), both at least 1.
        ``ValueError``, naming the argument, for a wrong dtype, rank or shape."""
        weights = _check_array("weights", weights, np.float32, "(channels, baselines)",
                               lambda s: len(s) == 2 and s[0] >= 1 and s[1] >= 1)  # fmt: skip
        with np.errstate(all="ignore"):
            ok = (weights > 0) & (weights < np.inf)
            m = np.where(ok, weights, np.float32(0)).max(axis=1)
            weights_channel = m / np.float32(255)
            t = weights / weights_channel[:, np.newaxis]
            positive = weights > 0
            # (rint only of what is used: a t that is NaN or 255 and more is replaced first)
            rounded = np.rint(np.where(positive & (t < 255), t, np.float32(1)))
            q = np.where(t >= 255, np.float32(255), np.maximum(rounded, np.float32(1)))
            weights8 = np.where(positive, q, np.float32(0)).astype(np.uint8)
        assert weights_channel.dtype == np.float32 and t.dtype == np.float32
        return weights8, weights_channel

    @staticmethod
    def expand(weights8: np.ndarray, weights_channel: np.ndarray) -> np.ndarray:
        """The consumer's side: ``float32(weights8) * weights_channel`` of its row, float32
        (channels, baselines). ``ValueError`` unless `weights8` is uint8 (channels, baselines)
        and `weights_channel` float32 (channels,)."""
        weights8 = _check_array("weights8", weights8, np.uint8, "(channels, baselines)",
                                lambda s: len(s) == 2)  # fmt: skip
        weights_channel = _check_array("weights_channel", weights_channel, np.float32,
                                       "(channels,)", lambda s: s == weights8.shape[:1])  # fmt: skip
        with np.errstate(all="ignore"):
            return weights8.astype(np.float32) * weights_channel[:, np.newaxis]


class ApplyGainsHost:
    """Per-input gain corrections applied to averaged visibilities, with the weights scaled to
    match and the samples without a correction flagged: what every consumer of calibrated data
    wants between :class:`AveragerHost` and the 2-D flagger or :class:`CompressWeightsHost`. No
    reference counterpart; this class is the definition that the device operation
    (:class:`.ingest.ApplyGainsTemplate`) matches bit for bit.

    ``gains[c, i]`` is the correction that *multiplies*: a caller with solved gains inverts them
    and combines bandpass, delay and gain on that small array first. ``inputs[j]`` names the two
    inputs ``(a, b)`` of baseline ``j``. Per channel ``c`` and baseline ``j``, every float step
    one float32 operation, rounded once (a multiply, then an add, never an fma; real and
    imaginary parts apart, not a complex multiply)::

        inr = 0 <= a < n_inputs and 0 <= b < n_inputs
        ga, gb = gains[c, a], gains[c, b]                 (not looked up unless inr)
        cr = ga.re*gb.re + ga.im*gb.im;  ci = ga.im*gb.re - ga.re*gb.im        (ga * conj(gb))
        ok = inr and cr is not NaN and ci is not NaN
        p  = cr*cr + ci*ci
        out_vis     = ok ? (v.re*cr - v.im*ci, v.re*ci + v.im*cr) : v
        out_weights = ok and p > 0 ? w / p : 0
        out_flags   = flags | (ok ? 0 : flag_value)

    What follows from it:

    * Without a correction (a NaN in it, or an index outside the gains; any int32 is allowed in
      `inputs`) the visibility passes through bit for bit, the weight becomes 0 and the sample
      is flagged.
    * Infinities and denormals go through as IEEE gives them: an infinite ``p`` makes a finite
      weight 0, and a correction whose parts subtract to ``inf - inf`` is a NaN correction.
    * An autocorrelation (``a == b``) with a finite gain has ``ci == +0`` exactly.
    * A zero correction (or one whose ``p`` underflows to 0) gives weight 0, "no data" as
      :class:`AveragerHost` reads it, and no flag.

    Parameters
    ----------
    flag_value
        Bits set in ``out_flags`` of a sample without a correction, 1..255
        (:func:`check_flag_byte`)
    """

    MAX_INPUTS = 4096

    def __init__(self, flag_value: int = 128) -> None:
        self.flag_value = check_flag_byte("flag_value", flag_value)

    def __call__(self, vis: np.ndarray, gains: np.ndarray, inputs: np.ndarray,
                 weights: Optional[np.ndarray] = None, flags: Optional[np.ndarray] = None):  # fmt: skip
        """``(out_vis, out_weights or None, out_flags or None)`` for complex64 `vis` (channels,
        baselines), complex64 `gains` (channels, n_inputs), int32 `inputs` (baselines, 2),
        optional float32 `weights` and optional uint8 `flags` (both channels, baselines).
        ``ValueError``, naming the argument, for a wrong dtype, rank or shape (channels and
        baselines at least 1, n_inputs 1..4096). No argument is modified."""
        vis = _check_array("vis", vis, np.complex64, "(channels, baselines)",
                           lambda s: len(s) == 2 and s[0] >= 1 and s[1] >= 1)  # fmt: skip
        channels, baselines = vis.shape
        gains = _check_array("gains", gains, np.complex64, "(channels, n_inputs), n_inputs 1..4096",
                             lambda s: len(s) == 2 and s[0] == channels
                             and 1 <= s[1] <= self.MAX_INPUTS)  # fmt: skip
        inputs = _check_array("inputs", inputs, np.int32, "(baselines, 2)",
                              lambda s: s == (baselines, 2))  # fmt: skip
        if weights is not None:
            weights = _check_array("weights", weights, np.float32, "(channels, baselines)",
                                   lambda s: s == vis.shape)  # fmt: skip
        if flags is not None:
            flags = _check_array("flags", flags, np.uint8, "(channels, baselines)",
                                 lambda s: s == vis.shape)  # fmt: skip
        n_inputs = gains.shape[1]
        inr = ((inputs >= 0) & (inputs < n_inputs)).all(axis=1)
        ga = gains[:, np.where(inr, inputs[:, 0], 0)]
        gb = gains[:, np.where(inr, inputs[:, 1], 0)]
        with np.errstate(all="ignore"):
            cr = ga.real * gb.real + ga.imag * gb.imag
            ci = ga.imag * gb.real - ga.real * gb.imag
            ok = inr[np.newaxis, :] & ~np.isnan(cr) & ~np.isnan(ci)
            p = cr * cr + ci * ci
            out_vis = np.empty((channels, baselines), np.complex64)
            out_vis.real[...] = np.where(ok, vis.real * cr - vis.imag * ci, vis.real)
            out_vis.imag[...] = np.where(ok, vis.real * ci + vis.imag * cr, vis.imag)
            assert cr.dtype == np.float32 and p.dtype == np.float32
            out_weights = None
            if weights is not None:
                scaled = ok & (p > 0)
                # (the divisor of a sample that gets no weight is 1, not p: no 0 / 0)
                out_weights = np.where(scaled, weights / np.where(scaled, p, np.float32(1)),
                                       np.float32(0))  # fmt: skip
        out_flags = None
        if flags is not None:
            out_flags = flags | np.where(ok, np.uint8(0), np.uint8(self.flag_value))
        return out_vis, out_weights, out_flags


class SolveGainsHost:
    """Per-input complex gains solved from averaged visibilities of a point source at the phase
    centre, channel by channel, with StEFCal (Salvini & Wijnholds 2014): what produces the
    gains that :class:`ApplyGainsHost` applies. No reference counterpart; this class is the
    definition that the device operation (:class:`.ingest.SolveGainsTemplate`) matches bit for
    bit.

    ``pairs[p, q]`` (only ``p < q`` is read) says where the baseline of inputs ``p`` and ``q``
    is: ``t > 0`` is baseline ``t - 1`` listed as ``(p, q)``, ``t < 0`` is baseline ``-t - 1``
    listed as ``(q, p)``, whose sample is conjugated, and ``0`` or ``|t| > baselines`` (any int32)
    is no baseline; :meth:`pair_table` builds it. A sample is *kept* when its entry is valid,
    neither part of ``v`` is NaN, ``w > 0`` (1 without `weights`) and ``flags & mask == 0``. Per
    channel a kept sample stores ``W[p][q] = W[q][p] = w``, ``A[p][q] = (w*v.re, w*v.im)``, the
    imaginary part negated for ``t < 0``, and ``A[q][p] = conj(A[p][q])``; everything else, the
    diagonal included, is +0. An input *has data* if its row of ``W`` has a positive entry.

    Every float step is one float32 operation, rounded once (a multiply, then an add, never an
    fma; real and imaginary parts apart; correctly rounded division and square root). From
    ``g = initial`` (or 1+0j), for ``k = 1 .. max_iterations``::

        s[q]   = g[q].re*g[q].re + g[q].im*g[q].im
        num[p] = sum_q (A.re*g.re - A.im*g.im, A.re*g.im + A.im*g.re)     (A = A[p][q], g = g[q])
        den[p] = sum_q W[p][q]*s[q]
        new[p] = den[p] > 0 ? (num.re/den, num.im/den) : g[p]
        k odd : g = new
        k even: g = ((new.re+g.re)*0.5, (new.im+g.im)*0.5)
                d = sum_p |g[p]-old[p]|^2,  n = sum_p |g[p]|^2      over the inputs that have data
                stop, converged, when d <= float32(tol*tol) * n

    with ``|x|^2 = x.re*x.re + x.im*x.im``. Every sum over q or p runs in blocks of
    :attr:`BLOCK` = 32 indices: within a block sequentially and ascending from +0, and the block
    sums are then added in ascending order. After the loop:

    * Referencing. If ``reference >= 0``, that input has data and ``m = sqrt(re*re + im*im)``
      of its gain is positive and finite, every gain is multiplied by ``(re/m, -im/m)`` and the
      reference's imaginary part is set to +0. Otherwise (``reference=-1`` included) status bit
      2 is set and the gains stay as they are.
    * With `corrections` the output is ``(g.re/s, -g.im/s)`` where ``s = |g|^2 > 0``, else NaN:
      what :class:`ApplyGainsHost` multiplies by.
    * An input without data comes out as NaN+NaNj, so that :class:`ApplyGainsHost` flags it.

    ``status`` bits: 1 not converged, 2 no input has data, 4 not referenced. Infinities go
    through as IEEE gives them, and a NaN criterion is "not converged".

    Parameters
    ----------
    max_iterations
        1..1000
    tol
        Relative change below which a channel stops, at least 0
    reference
        -1 (none) or the input whose gain is made real and positive
    mask
        Flag bits that exclude a sample, 0..255 (:func:`check_mask_byte`)
    corrections
        ``True``: return the reciprocal gains
    """

    MAX_INPUTS = 128
    MAX_ITERATIONS = 1000
    BLOCK = 32
    NOT_CONVERGED, NO_DATA, NOT_REFERENCED = 1, 2, 4
    _CHUNK = 32  # channels worked on at once (memory only)

    def __init__(self, max_iterations: int = 30, tol: float = 1e-5, reference: int = 0,
                 mask: int = 0xFF, corrections: bool = False) -> None:  # fmt: skip
        for name, value in (("max_iterations", max_iterations), ("reference", reference)):
            if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
                raise TypeError(f"{name} {value!r} is not an integer")
        if not 1 <= max_iterations <= self.MAX_ITERATIONS:
            raise ValueError(f"max_iterations must be 1..{self.MAX_ITERATIONS}")
        if not float(tol) >= 0:
            raise ValueError(f"tol {tol!r} must be at least 0")
        if not -1 <= reference < self.MAX_INPUTS:
            raise ValueError(f"reference must be -1..{self.MAX_INPUTS - 1}")
        self.max_iterations = int(max_iterations)
        self.tol = float(tol)
        with np.errstate(all="ignore"):
            self.tol2 = np.float32(self.tol * self.tol)
        self.reference = int(reference)
        self.mask = check_mask_byte("mask", mask)
        self.corrections = bool(corrections)

    @classmethod
    def check_n_inputs(cls, n_inputs) -> int:
        """`n_inputs` as an int in 1..:attr:`MAX_INPUTS` (``ValueError`` otherwise,
        ``TypeError`` for a value that is not an integer)."""
        if isinstance(n_inputs, (bool, np.bool_)) or not isinstance(n_inputs, (int, np.integer)):
            raise TypeError(f"n_inputs {n_inputs!r} is not an integer")
        if not 1 <= n_inputs <= cls.MAX_INPUTS:
            raise ValueError(f"n_inputs must be 1..{cls.MAX_INPUTS}")
        return int(n_inputs)

    @classmethod
    def pair_table(cls, inputs, n_inputs: int) -> np.ndarray:
        """The int32 (n_inputs, n_inputs) table of `inputs` (baselines x 2, as
        :class:`ApplyGainsHost` takes them). Autocorrelations and baselines with an entry
        outside ``0..n_inputs-1`` take no part; ``ValueError`` for a pair that is listed twice,
        in either order."""
        n_inputs = cls.check_n_inputs(n_inputs)
        inputs = np.asarray(inputs)
        if inputs.ndim != 2 or inputs.shape[1] != 2 or inputs.dtype.kind not in "iu":
            raise ValueError(f"inputs must be integers of shape (baselines, 2), not "
                             f"{inputs.dtype.name} {inputs.shape}")  # fmt: skip
        if len(inputs) >= 2**31:
            raise ValueError("inputs lists more than 2^31 - 1 baselines")
        table = np.zeros((n_inputs, n_inputs), np.int32)
        for j, (a, b) in enumerate(inputs.tolist()):
            if a == b or not (0 <= a < n_inputs and 0 <= b < n_inputs):
                continue
            p, q, entry = (a, b, j + 1) if a < b else (b, a, -(j + 1))
            if table[p, q] != 0:
                raise ValueError(f"inputs lists the pair ({p}, {q}) twice: baselines "
                                 f"{abs(int(table[p, q])) - 1} and {j}")  # fmt: skip
            table[p, q] = entry
        return table

    @classmethod
    def _block_sum(cls, terms: np.ndarray) -> np.ndarray:
        """float32 sums over the last axis in the order of the class docstring."""
        total = None
        for start in range(0, terms.shape[-1], cls.BLOCK):
            partial = np.zeros(terms.shape[:-1], np.float32)
            for i in range(start, min(start + cls.BLOCK, terms.shape[-1])):
                partial = partial + terms[..., i]
            total = partial if total is None else total + partial
        assert total.dtype == np.float32
        return total

    def __call__(self, vis: np.ndarray, pairs: np.ndarray, weights: Optional[np.ndarray] = None,
                 flags: Optional[np.ndarray] = None, initial: Optional[np.ndarray] = None):  # fmt: skip
        """``(gains, iterations, status)``: complex64 (channels, n_inputs), int32 (channels,)
        and uint8 (channels,), for complex64 `vis` (channels, baselines), int32 `pairs`
        (n_inputs, n_inputs), optional float32 `weights`, optional uint8 `flags` (both channels,
        baselines) and optional complex64 `initial` (channels, n_inputs). ``ValueError``, naming
        the argument, for a wrong dtype, rank or shape (channels and baselines at least 1,
        n_inputs 1..:attr:`MAX_INPUTS`) and for a `reference` that is not below n_inputs. No
        argument is modified."""
        vis = _check_array("vis", vis, np.complex64, "(channels, baselines)",
                           lambda s: len(s) == 2 and s[0] >= 1 and s[1] >= 1)  # fmt: skip
        channels, baselines = vis.shape
        pairs = _check_array("pairs", pairs, np.int32,
                             f"(n_inputs, n_inputs), n_inputs 1..{self.MAX_INPUTS}",
                             lambda s: len(s) == 2 and s[0] == s[1]
                             and 1 <= s[0] <= self.MAX_INPUTS)  # fmt: skip
        n = pairs.shape[0]
        if weights is not None:
            weights = _check_array("weights", weights, np.float32, "(channels, baselines)",
                                   lambda s: s == vis.shape)  # fmt: skip
        if flags is not None:
            flags = _check_array("flags", flags, np.uint8, "(channels, baselines)",
                                 lambda s: s == vis.shape)  # fmt: skip
        if initial is not None:
            initial = _check_array("initial", initial, np.complex64, "(channels, n_inputs)",
                                   lambda s: s == (channels, n))  # fmt: skip
        if self.reference >= n:
            raise ValueError(f"reference must be -1 or 0..n_inputs-1 = {n - 1}, not {self.reference}")
        gains = np.empty((channels, n), np.complex64)
        iterations = np.empty(channels, np.int32)
        status = np.empty(channels, np.uint8)
        for c0 in range(0, channels, self._CHUNK):
            rows = slice(c0, min(c0 + self._CHUNK, channels))
            gains[rows], iterations[rows], status[rows] = self._solve(
                vis[rows], pairs, None if weights is None else weights[rows],
                None if flags is None else flags[rows],
                None if initial is None else initial[rows])  # fmt: skip
        return gains, iterations, status

    def _matrix(self, vis, pairs, weights, flags):
        """``A.re, A.im, W`` (channels, n, n) float32 of the class docstring."""
        channels, baselines = vis.shape
        n = pairs.shape[0]
        f32 = np.float32
        p, q = np.triu_indices(n, 1)
        t = pairs[p, q].astype(np.int64)
        valid = (t != 0) & (np.abs(t) <= baselines)
        j = np.where(valid, np.abs(t) - 1, 0)
        v = vis[:, j]
        w = np.ones(v.shape, f32) if weights is None else weights[:, j]
        kept = valid[np.newaxis, :] & ~np.isnan(v.real) & ~np.isnan(v.imag) & (w > 0)
        if flags is not None:
            kept &= (flags[:, j] & np.uint8(self.mask)) == 0
        zero = f32(0)
        a_im = w * v.imag
        a_im = np.where(kept, np.where(t < 0, -a_im, a_im), zero)
        a_re = np.where(kept, w * v.real, zero)
        big_re, big_im, big_w = (np.zeros((channels, n, n), f32) for _ in range(3))
        big_re[:, p, q] = a_re
        big_re[:, q, p] = a_re
        big_im[:, p, q] = a_im
        big_im[:, q, p] = np.where(kept, -a_im, zero)
        big_w[:, p, q] = big_w[:, q, p] = np.where(kept, w, zero)
        return big_re, big_im, big_w

    def _solve(self, vis, pairs, weights, flags, initial):
        channels = vis.shape[0]
        n = pairs.shape[0]
        f32 = np.float32
        half, zero, one = f32(0.5), f32(0), f32(1)
        bsum = self._block_sum
        with np.errstate(all="ignore"):
            a_re, a_im, w = self._matrix(vis, pairs, weights, flags)
            has = (w > 0).any(axis=2)
            if initial is None:
                g_re, g_im = np.ones((channels, n), f32), np.zeros((channels, n), f32)
            else:
                g_re, g_im = np.array(initial.real), np.array(initial.imag)  # (copies)
            iterations = np.zeros(channels, np.int32)
            converged = np.zeros(channels, bool)
            for k in range(1, self.max_iterations + 1):
                act = np.flatnonzero(~converged)
                if not act.size:
                    break
                gr, gi = g_re[act], g_im[act]
                s = gr * gr + gi * gi
                gr_q, gi_q = gr[:, np.newaxis, :], gi[:, np.newaxis, :]
                ar, ai = a_re[act], a_im[act]
                num_re = bsum(ar * gr_q - ai * gi_q)
                num_im = bsum(ar * gi_q + ai * gr_q)
                den = bsum(w[act] * s[:, np.newaxis, :])
                pos = den > 0
                safe = np.where(pos, den, one)  # (no 0 / 0 where the quotient is not used)
                new_re = np.where(pos, num_re / safe, gr)
                new_im = np.where(pos, num_im / safe, gi)
                if k % 2:
                    g_re[act], g_im[act] = new_re, new_im
                else:
                    new_re = (new_re + gr) * half
                    new_im = (new_im + gi) * half
                    dr, di = new_re - gr, new_im - gi
                    d = bsum(np.where(has[act], dr * dr + di * di, zero))
                    norm = bsum(np.where(has[act], new_re * new_re + new_im * new_im, zero))
                    g_re[act], g_im[act] = new_re, new_im
                    converged[act] = d <= self.tol2 * norm
                iterations[act] = k
            status = np.where(converged, 0, self.NOT_CONVERGED).astype(np.uint8)
            status[~has.any(axis=1)] |= np.uint8(self.NO_DATA)
            # referencing
            referenced = np.zeros(channels, bool)
            if self.reference >= 0:
                r_re, r_im = g_re[:, self.reference], g_im[:, self.reference]
                m = np.sqrt(r_re * r_re + r_im * r_im)
                referenced = has[:, self.reference] & (m > 0) & np.isfinite(m)
                safe = np.where(referenced, m, one)
                u_re, u_im = (r_re / safe)[:, np.newaxis], (-r_im / safe)[:, np.newaxis]
                rows = referenced[:, np.newaxis]
                turned_re = np.where(rows, g_re * u_re - g_im * u_im, g_re)
                turned_im = np.where(rows, g_re * u_im + g_im * u_re, g_im)
                g_re, g_im = turned_re, turned_im
                g_im[:, self.reference] = np.where(referenced, zero, g_im[:, self.reference])
            status[~referenced] |= np.uint8(self.NOT_REFERENCED)
            if self.corrections:
                s = g_re * g_re + g_im * g_im
                pos = s > 0
                safe = np.where(pos, s, one)
                g_re = np.where(pos, g_re / safe, f32(np.nan))
                g_im = np.where(pos, -g_im / safe, f32(np.nan))
            gains = np.empty((channels, n), np.complex64)
            gains.real[...] = np.where(has, g_re, f32(np.nan))
            gains.imag[...] = np.where(has, g_im, f32(np.nan))
            assert g_re.dtype == f32 and g_im.dtype == f32
        return gains, iterations, status


class SolveGainsLargeHost(SolveGainsHost):
    """:class:`SolveGainsHost` for up to 512 inputs: the same arguments, ``pair_table``,
    arithmetic and results, with up to 16 block sums of :attr:`BLOCK` = 32 indices per row and
    in the convergence sums instead of 4. Up to 128 inputs the results are bit for bit those of
    :class:`SolveGainsHost`. No reference counterpart; this class is the definition that the
    device operation (:class:`.ingest.SolveGainsLargeTemplate`) matches bit for bit."""

    MAX_INPUTS = 512
    _CHUNK = 8  # (a channel's three matrices are 3 MiB at 512 inputs)


class SolveJonesHost(SolveGainsHost):
    """Per-antenna 2x2 Jones matrices solved from averaged visibilities of an unpolarised unit
    source at the phase centre, channel by channel, with the full-polarisation StEFCal step
    (Salvini & Wijnholds 2014, section 4): the leakage solve that :class:`SolveGainsHost`, which
    treats the two feeds of a dish as unrelated inputs, cannot do. No reference counterpart;
    this class is the definition that the device operation (:class:`.ingest.SolveJonesTemplate`)
    matches bit for bit.

    ``n_inputs`` is even, 2..128; input ``2a + i`` is feed ``i`` of antenna ``a``. The arguments
    are those of :class:`SolveGainsHost`, with the same kept-sample rule and the same rules for
    an entry of ``pairs``, and one more: an entry whose two inputs belong to one antenna
    (``p // 2 == q // 2``, the cross-feed autocorrelation) is treated as 0. ``A``, ``W`` and
    "has data" are built as there. ``initial`` and the result ``jones`` are complex64
    (channels, n_inputs, 2): row ``p = 2a + i`` is row ``i`` of antenna ``a``'s Jones matrix,
    ``z_p = (J_a[i][0], J_a[i][1])``, and the model is ``V[p][q] = z_p[0] conj(z_q[0]) +
    z_p[1] conj(z_q[1])``. Without `initial` every matrix starts as the identity.

    Every float step is one float32 operation, rounded once, in the order written (never an
    fma; real and imaginary parts apart; correctly rounded division and square root). With
    ``x = z_q[0]``, ``y = z_q[1]``, ``|x|^2 = x.re*x.re + x.im*x.im``, ``a*b = (a.re*b.re -
    a.im*b.im, a.re*b.im + a.im*b.re)`` and ``a*conj(b) = (a.re*b.re + a.im*b.im, a.im*b.re -
    a.re*b.im)``, for ``k = 1 .. max_iterations``::

        s00[q] = |x|^2;  s11[q] = |y|^2;  s01[q] = y*conj(x)
        num0[p] = sum_q A[p][q]*x;  num1[p] = sum_q A[p][q]*y
        h00[p] = sum_q W[p][q]*s00[q];  h11[p] = sum_q W[p][q]*s11[q]
        h01[p] = sum_q (W[p][q]*s01[q].re, W[p][q]*s01[q].im)
        det = h00*h11 - |h01|^2
        det > 0:  c = num1*conj(h01);  e = num0*h01
                  new0 = ((num0.re*h11 - c.re)/det, (num0.im*h11 - c.im)/det)
                  new1 = ((num1.re*h00 - e.re)/det, (num1.im*h00 - e.im)/det)
        else:     new = z_p                                     (a NaN det is not above 0)
        k odd : z = new
        k even: z = ((new.re + z.re)*0.5, (new.im + z.im)*0.5) for both elements,
                d = sum_p (|z_p[0]-old_p[0]|^2 + |z_p[1]-old_p[1]|^2)
                n = sum_p (|z_p[0]|^2 + |z_p[1]|^2)             over the inputs that have data
                stop, converged, when d <= float32(tol*tol) * n

    Every sum over q or p runs in the blocks of 32 of :class:`SolveGainsHost`. After the loop:

    * Referencing. `reference` is an antenna, or -1. With ``R = [[a, b], [c, d]]`` its matrix
      (``a, b = z_2r``; ``c, d = z_2r+1``), ``D = a*d - b*c`` and ``m = sqrt(|D|^2)``: if both
      of its inputs have data and m is positive and finite, then ``e = (D.re/m, D.im/m)``,
      ``B = [[a + e*conj(d), b - e*conj(c)], [c - e*conj(b), d + e*conj(a)]]``,
      ``t = sqrt(sqrt(|B00*B11 - B01*B10|^2))``, ``U[i][j] = (B[i][j].re/t, B[i][j].im/t)`` and
      every row becomes ``(x*conj(U00) + y*conj(U01), x*conj(U10) + y*conj(U11))``. U is the
      unitary factor of R's polar decomposition, so the reference's matrix becomes Hermitian
      and positive; the imaginary parts of its diagonal are set to +0. Otherwise status bit 2
      is set and nothing is rotated. For an unpolarised source the data fix the matrices only
      up to one common unitary factor on the right: this choice of U is a convention that the
      data cannot check.
    * With `corrections`, each antenna's matrix ``[[a, b], [c, d]]`` is replaced by its inverse:
      ``D = a*d - b*c``, ``s = |D|^2``, ``i = (D.re/s, -D.im/s)`` and ``[[d*i, -(b*i)],
      [-(c*i), a*i]]`` where ``s > 0`` and both inputs have data, else NaN in all four.
    * Without corrections only the rows of inputs without data are NaN+NaNj.

    ``status`` bits: 1 not converged, 2 no input has data, 4 not referenced, 8 in the last
    iteration an input with data kept its row because ``det`` was not above 0.

    Parameters
    ----------
    max_iterations, tol, mask
        As for :class:`SolveGainsHost`
    reference
        -1 (none) or the antenna whose matrix is made Hermitian and positive, up to 63
    corrections
        ``True``: return the inverse matrices
    """

    MAX_ANTENNAS = SolveGainsHost.MAX_INPUTS // 2
    DET_NOT_POSITIVE = 8

    def __init__(self, max_iterations: int = 30, tol: float = 1e-5, reference: int = 0,
                 mask: int = 0xFF, corrections: bool = False) -> None:  # fmt: skip
        if isinstance(reference, (int, np.integer)) and not isinstance(reference, (bool, np.bool_)):
            if not -1 <= reference < self.MAX_ANTENNAS:
                raise ValueError(f"reference must be -1..{self.MAX_ANTENNAS - 1}")
        super().__init__(max_iterations, tol, reference, mask, corrections)

    @classmethod
    def check_n_inputs(cls, n_inputs) -> int:
        """`n_inputs` as an even int in 2..128 (``ValueError`` otherwise, ``TypeError`` for a
        value that is not an integer)."""
        if isinstance(n_inputs, (bool, np.bool_)) or not isinstance(n_inputs, (int, np.integer)):
            raise TypeError(f"n_inputs {n_inputs!r} is not an integer")
        if not 2 <= n_inputs <= cls.MAX_INPUTS or n_inputs % 2:
            raise ValueError(f"n_inputs must be even and 2..{cls.MAX_INPUTS}")
        return int(n_inputs)

    def __call__(self, vis: np.ndarray, pairs: np.ndarray, weights: Optional[np.ndarray] = None,
                 flags: Optional[np.ndarray] = None, initial: Optional[np.ndarray] = None):  # fmt: skip
        """``(jones, iterations, status)``: complex64 (channels, n_inputs, 2), int32
        (channels,) and uint8 (channels,), for complex64 `vis` (channels, baselines), int32
        `pairs` (n_inputs, n_inputs), optional float32 `weights`, optional uint8 `flags` (both
        channels, baselines) and optional complex64 `initial` (channels, n_inputs, 2).
        ``ValueError``, naming the argument, for a wrong dtype, rank or shape (channels and
        baselines at least 1, n_inputs even and 2..128) and for a `reference` that is not
        below n_inputs / 2. No argument is modified."""
        vis = _check_array("vis", vis, np.complex64, "(channels, baselines)",
                           lambda s: len(s) == 2 and s[0] >= 1 and s[1] >= 1)  # fmt: skip
        channels = vis.shape[0]
        pairs = _check_array("pairs", pairs, np.int32,
                             "(n_inputs, n_inputs), n_inputs even and 2..128",
                             lambda s: len(s) == 2 and s[0] == s[1] and s[0] % 2 == 0
                             and 2 <= s[0] <= self.MAX_INPUTS)  # fmt: skip
        n = pairs.shape[0]
        if weights is not None:
            weights = _check_array("weights", weights, np.float32, "(channels, baselines)",
                                   lambda s: s == vis.shape)  # fmt: skip
        if flags is not None:
            flags = _check_array("flags", flags, np.uint8, "(channels, baselines)",
                                 lambda s: s == vis.shape)  # fmt: skip
        if initial is not None:
            initial = _check_array("initial", initial, np.complex64, "(channels, n_inputs, 2)",
                                   lambda s: s == (channels, n, 2))  # fmt: skip
        if self.reference >= n // 2:
            raise ValueError(f"reference must be -1 or 0..n_inputs/2-1 = {n // 2 - 1}, "
                             f"not {self.reference}")  # fmt: skip
        # an entry within one antenna is no baseline (the lower triangle is never read)
        index = np.arange(n) // 2
        pairs = np.where(index[:, np.newaxis] == index[np.newaxis, :], np.int32(0), pairs)
        jones = np.empty((channels, n, 2), np.complex64)
        iterations = np.empty(channels, np.int32)
        status = np.empty(channels, np.uint8)
        for c0 in range(0, channels, self._CHUNK):
            rows = slice(c0, min(c0 + self._CHUNK, channels))
            jones[rows], iterations[rows], status[rows] = self._solve(
                vis[rows], pairs, None if weights is None else weights[rows],
                None if flags is None else flags[rows],
                None if initial is None else initial[rows])  # fmt: skip
        return jones, iterations, status

    @staticmethod
    def _mul(a, b):
        """``a*b`` of the class docstring on (re, im) pairs."""
        return a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]

    @staticmethod
    def _mul_conj(a, b):
        """``a*conj(b)`` of the class docstring on (re, im) pairs."""
        return a[0] * b[0] + a[1] * b[1], a[1] * b[0] - a[0] * b[1]

    @staticmethod
    def _norm2(a):
        return a[0] * a[0] + a[1] * a[1]

    def _solve(self, vis, pairs, weights, flags, initial):
        channels = vis.shape[0]
        n = pairs.shape[0]
        f32 = np.float32
        half, zero, one, nan = f32(0.5), f32(0), f32(1), f32(np.nan)
        bsum, mul, mul_conj, norm2 = self._block_sum, self._mul, self._mul_conj, self._norm2
        with np.errstate(all="ignore"):
            a_re, a_im, w = self._matrix(vis, pairs, weights, flags)
            has = (w > 0).any(axis=2)
            # z[e][part]: element e of every row, real and imaginary parts apart
            if initial is None:
                even = (np.arange(n) % 2 == 0)[np.newaxis, :].repeat(channels, axis=0)
                z = [[even.astype(f32), np.zeros((channels, n), f32)],
                     [(~even).astype(f32), np.zeros((channels, n), f32)]]  # fmt: skip
            else:
                z = [[np.array(initial[:, :, e].real), np.array(initial[:, :, e].imag)]
                     for e in range(2)]  # fmt: skip
            iterations = np.zeros(channels, np.int32)
            converged = np.zeros(channels, bool)
            stuck = np.zeros(channels, bool)
            for k in range(1, self.max_iterations + 1):
                act = np.flatnonzero(~converged)
                if not act.size:
                    break
                x = (z[0][0][act], z[0][1][act])
                y = (z[1][0][act], z[1][1][act])
                s00, s11, s01 = norm2(x), norm2(y), mul_conj(y, x)
                a = (a_re[act], a_im[act])
                wa = w[act]

                def over_q(v):
                    return v[:, np.newaxis, :]

                num0 = tuple(bsum(t) for t in mul(a, (over_q(x[0]), over_q(x[1]))))
                num1 = tuple(bsum(t) for t in mul(a, (over_q(y[0]), over_q(y[1]))))
                h00, h11 = bsum(wa * over_q(s00)), bsum(wa * over_q(s11))
                h01 = (bsum(wa * over_q(s01[0])), bsum(wa * over_q(s01[1])))
                det = h00 * h11 - norm2(h01)
                pos = det > 0
                safe = np.where(pos, det, one)  # (no 0 / 0 where the quotient is not used)
                c, e = mul_conj(num1, h01), mul(num0, h01)
                new = [[np.where(pos, (num0[i] * h11 - c[i]) / safe, x[i]) for i in range(2)],
                       [np.where(pos, (num1[i] * h00 - e[i]) / safe, y[i]) for i in range(2)]]
                stuck[act] = (has[act] & ~pos).any(axis=1)
                if k % 2 == 0:
                    old = (x, y)
                    new = [[(new[e][i] + old[e][i]) * half for i in range(2)] for e in range(2)]
                    diff = [(new[e][0] - old[e][0], new[e][1] - old[e][1]) for e in range(2)]
                    d = bsum(np.where(has[act], norm2(diff[0]) + norm2(diff[1]), zero))
                    norm = bsum(np.where(has[act], norm2(new[0]) + norm2(new[1]), zero))
                    converged[act] = d <= self.tol2 * norm
                for e in range(2):
                    for i in range(2):
                        z[e][i][act] = new[e][i]
                iterations[act] = k
            status = np.where(converged, 0, self.NOT_CONVERGED).astype(np.uint8)
            status[~has.any(axis=1)] |= np.uint8(self.NO_DATA)
            status[stuck] |= np.uint8(self.DET_NOT_POSITIVE)
            x, y = (z[0][0], z[0][1]), (z[1][0], z[1][1])
            # referencing
            referenced = np.zeros(channels, bool)
            if self.reference >= 0:
                r0, r1 = 2 * self.reference, 2 * self.reference + 1

                def at(v, p):
                    return v[0][:, p], v[1][:, p]

                ra, rb, rc, rd = at(x, r0), at(y, r0), at(x, r1), at(y, r1)
                ad, bc = mul(ra, rd), mul(rb, rc)
                big_d = (ad[0] - bc[0], ad[1] - bc[1])
                m = np.sqrt(norm2(big_d))
                referenced = has[:, r0] & has[:, r1] & (m > 0) & np.isfinite(m)
                safe = np.where(referenced, m, one)
                e = (big_d[0] / safe, big_d[1] / safe)
                ed, ec, eb, ea = mul_conj(e, rd), mul_conj(e, rc), mul_conj(e, rb), mul_conj(e, ra)
                b00 = (ra[0] + ed[0], ra[1] + ed[1])
                b01 = (rb[0] - ec[0], rb[1] - ec[1])
                b10 = (rc[0] - eb[0], rc[1] - eb[1])
                b11 = (rd[0] + ea[0], rd[1] + ea[1])
                p00, p01 = mul(b00, b11), mul(b01, b10)
                t = np.sqrt(np.sqrt(norm2((p00[0] - p01[0], p00[1] - p01[1]))))
                t = np.where(referenced, t, one)
                u = [tuple((part / t)[:, np.newaxis] for part in b) for b in (b00, b01, b10, b11)]
                rows = referenced[:, np.newaxis]
                turned = []
                for u0, u1 in ((u[0], u[1]), (u[2], u[3])):
                    first, second = mul_conj(x, u0), mul_conj(y, u1)
                    turned.append((first[0] + second[0], first[1] + second[1]))
                x = tuple(np.where(rows, turned[0][i], x[i]) for i in range(2))
                y = tuple(np.where(rows, turned[1][i], y[i]) for i in range(2))
                x[1][:, r0] = np.where(referenced, zero, x[1][:, r0])
                y[1][:, r1] = np.where(referenced, zero, y[1][:, r1])
            status[~referenced] |= np.uint8(self.NOT_REFERENCED)
            if self.corrections:
                ja, jb = (x[0][:, 0::2], x[1][:, 0::2]), (y[0][:, 0::2], y[1][:, 0::2])
                jc, jd = (x[0][:, 1::2], x[1][:, 1::2]), (y[0][:, 1::2], y[1][:, 1::2])
                ad, bc = mul(ja, jd), mul(jb, jc)
                big_d = (ad[0] - bc[0], ad[1] - bc[1])
                s = norm2(big_d)
                pos = (s > 0) & has[:, 0::2] & has[:, 1::2]
                safe = np.where(pos, s, one)
                inv = (big_d[0] / safe, -big_d[1] / safe)
                di, bi, ci, ai = mul(jd, inv), mul(jb, inv), mul(jc, inv), mul(ja, inv)
                x = tuple(np.empty((channels, n), f32) for _ in range(2))
                y = tuple(np.empty((channels, n), f32) for _ in range(2))
                for i in range(2):
                    x[i][:, 0::2] = np.where(pos, di[i], nan)
                    y[i][:, 0::2] = np.where(pos, -bi[i], nan)
                    x[i][:, 1::2] = np.where(pos, -ci[i], nan)
                    y[i][:, 1::2] = np.where(pos, ai[i], nan)
            else:
                x = tuple(np.where(has, part, nan) for part in x)
                y = tuple(np.where(has, part, nan) for part in y)
            jones = np.empty((channels, n, 2), np.complex64)
            jones.real[:, :, 0], jones.imag[:, :, 0] = x
            jones.real[:, :, 1], jones.imag[:, :, 1] = y
            assert all(part.dtype == f32 for part in x + y)
        return jones, iterations, status


class ApplyJonesHost:
    """Per-antenna 2x2 Jones corrections applied to averaged visibilities, ``C_a V_ab C_b^H``
    on the four products of every antenna pair, with the weights propagated and the samples
    without a correction flagged: what :class:`ApplyGainsHost` does for one complex number per
    input, for the matrices that :class:`SolveJonesHost` leaves with ``corrections=True``. No
    reference counterpart; this class is the definition that the device operation
    (:class:`.ingest.ApplyJonesTemplate`) matches bit for bit.

    ``jones`` is complex64 (channels, n_inputs, 2) as :class:`SolveJonesHost` writes it: row
    ``2a + i`` is row ``i`` of antenna ``a``'s matrix ``C_a``; ``n_inputs`` is even, 2..2048.
    The unit of work is a *quad*, the four products of one antenna pair: ``quad_antennas[q]``
    is ``(a, b)`` and ``quads[q]`` is ``(t00, t01, t10, t11)``, where the entry ``t`` at
    ``(m, n)`` is in the convention of ``pairs`` (:class:`SolveGainsHost`): ``t > 0`` is
    baseline ``t - 1`` listed as ``(2a+m, 2b+n)``, ``t < 0`` is baseline ``-t - 1`` listed the
    other way round, whose imaginary part is negated on load and again on store, and ``0`` or
    ``|t| > baselines`` (any int32) is absent and forms no address. In a quad with ``a == b``
    (a dish's own products) an absent ``(1, 0)`` beside a present ``(0, 1)`` reads as the
    conjugate of that sample with its ``w`` and ``f``, and the other way round; nothing is
    stored for an absent entry. :meth:`quad_table` builds both arrays.

    Per channel ``c`` and quad, every float step is one float32 operation, rounded once (a
    multiply, then an add, never an fma; real and imaginary parts apart; correctly rounded
    division), sums added in the order written, with ``x*y = (x.re*y.re - x.im*y.im,
    x.re*y.im + x.im*y.re)`` and ``x*conj(y) = (x.re*y.re + x.im*y.im, x.im*y.re -
    x.re*y.im)``::

        complete = 0 <= a < n_ant and 0 <= b < n_ant and all four sources present
                   (a stand-in counts)
        ok       = complete and none of the 16 floats of rows 2a, 2a+1, 2b, 2b+1 of jones[c]
                   is NaN            (jones is not looked up unless both antennas are in range)
        S[m][n]  = source sample (re, t<0 ? -im : im);  w[m][n] (1 without weights);  f[m][n]
        T[i][n]  = C_a[i][0]*S[0][n] + C_a[i][1]*S[1][n]
        O[i][k]  = T[i][0]*conj(C_b[k][0]) + T[i][1]*conj(C_b[k][1])
        all_w    = every w[m][n] > 0                                     (a NaN is not)
        r[m][n]  = 1 / w[m][n];   al[i][m] = |C_a[i][m]|^2;   be[k][n] = |C_b[k][n]|^2
        u[i][n]  = al[i][0]*r[0][n] + al[i][1]*r[1][n]
        var[i][k]= u[i][0]*be[k][0] + u[i][1]*be[k][1]
        F        = OR of f over the present sources
        for every entry (i, k) that is present in `quads` itself, at baseline j:
          out_vis[c][j]     = ok ? (O.re, t<0 ? -O.im : O.im) : vis[c][j]   (the input's bits)
          out_weights[c][j] = ok and all_w and var[i][k] > 0 ? 1/var[i][k] : 0
          out_flags[c][j]   = F | (ok ? 0 : flag_value)

    ``var[i][k]`` is the variance of ``O[i][k]`` for independent sources of variance ``1/w``.
    What follows from it:

    * A flag or a missing weight on one product reaches all four: a polarimetric correction
      needs the whole coherency matrix.
    * An incomplete quad or a NaN matrix passes its visibilities through bit for bit, with
      weight 0 and `flag_value`.
    * Infinities, denormals and NaN samples go as IEEE gives them.
    * An autocorrelation does not stay exactly real.
    * A baseline in no quad is not written at all: here its outputs are the inputs; on the
      device it keeps its values in place, and out of place its output elements are untouched.

    Parameters
    ----------
    flag_value
        Bits set in ``out_flags`` of a sample without a correction, 1..255
        (:func:`check_flag_byte`)
    """

    MAX_INPUTS = 2048

    def __init__(self, flag_value: int = 128) -> None:
        self.flag_value = check_flag_byte("flag_value", flag_value)

    @classmethod
    def check_n_inputs(cls, n_inputs) -> int:
        """`n_inputs` as an even int in 2..2048 (``ValueError`` otherwise, ``TypeError`` for a
        value that is not an integer)."""
        if isinstance(n_inputs, (bool, np.bool_)) or not isinstance(n_inputs, (int, np.integer)):
            raise TypeError(f"n_inputs {n_inputs!r} is not an integer")
        if not 2 <= n_inputs <= cls.MAX_INPUTS or n_inputs % 2:
            raise ValueError(f"n_inputs must be even and 2..{cls.MAX_INPUTS}")
        return int(n_inputs)

    @classmethod
    def quad_table(cls, inputs, n_inputs: int) -> Tuple[np.ndarray, np.ndarray]:
        """``(quad_antennas, quads)``, int32 (n_quads, 2) and (n_quads, 4), of `inputs`
        (baselines x 2, as :meth:`SolveGainsHost.pair_table` takes them). A baseline ``(p, q)``
        with ``p // 2 <= q // 2`` is entry ``(p % 2, q % 2)`` of quad ``(p // 2, q // 2)``,
        positive; any other is entry ``(q % 2, p % 2)`` of quad ``(q // 2, p // 2)``, negative.
        A baseline with an index outside ``0..n_inputs-1`` belongs to no quad. The quads are
        ordered by the smallest baseline index they name. ``ValueError`` for an entry that is
        filled twice and when no baseline was placed."""
        n_inputs = cls.check_n_inputs(n_inputs)
        inputs = np.asarray(inputs)
        if inputs.ndim != 2 or inputs.shape[1] != 2 or inputs.dtype.kind not in "iu":
            raise ValueError(f"inputs must be integers of shape (baselines, 2), not "
                             f"{inputs.dtype.name} {inputs.shape}")  # fmt: skip
        if len(inputs) >= 2**31:
            raise ValueError("inputs lists more than 2^31 - 1 baselines")
        table = {}  # (a, b) -> its four entries; insertion order is the order of the quads
        for j, (p, q) in enumerate(inputs.tolist()):
            if not (0 <= p < n_inputs and 0 <= q < n_inputs):
                continue
            if p // 2 <= q // 2:
                key, entry, value = (p // 2, q // 2), 2 * (p % 2) + q % 2, j + 1
            else:
                key, entry, value = (q // 2, p // 2), 2 * (q % 2) + p % 2, -(j + 1)
            row = table.setdefault(key, [0, 0, 0, 0])
            if row[entry] != 0:
                raise ValueError(f"inputs lists the pair ({2 * key[0] + entry // 2}, "
                                 f"{2 * key[1] + entry % 2}) twice: baselines "
                                 f"{abs(row[entry]) - 1} and {j}")  # fmt: skip
            row[entry] = value
        if not table:
            raise ValueError("inputs lists no baseline between inputs 0..n_inputs-1")
        quad_antennas = np.array(list(table.keys()), np.int32).reshape(-1, 2)
        quads = np.array(list(table.values()), np.int32).reshape(-1, 4)
        return quad_antennas, quads

    @staticmethod
    def _add(a, b):
        """``a + b`` on (re, im) pairs."""
        return a[0] + b[0], a[1] + b[1]

    def __call__(self, vis: np.ndarray, jones: np.ndarray, quad_antennas: np.ndarray,
                 quads: np.ndarray, weights: Optional[np.ndarray] = None,
                 flags: Optional[np.ndarray] = None):  # fmt: skip
        """``(out_vis, out_weights or None, out_flags or None)`` for complex64 `vis` (channels,
        baselines), complex64 `jones` (channels, n_inputs, 2), int32 `quad_antennas`
        (n_quads, 2), int32 `quads` (n_quads, 4), optional float32 `weights` and optional uint8
        `flags` (both channels, baselines). ``ValueError``, naming the argument, for a wrong
        dtype, rank or shape (channels, baselines and n_quads at least 1, n_inputs even and
        2..2048), and if `quads` names one baseline in two present entries. No argument is
        modified."""
        vis = _check_array("vis", vis, np.complex64, "(channels, baselines)",
                           lambda s: len(s) == 2 and s[0] >= 1 and s[1] >= 1)  # fmt: skip
        channels, baselines = vis.shape
        jones = _check_array("jones", jones, np.complex64,
                             "(channels, n_inputs, 2), n_inputs even and 2..2048",
                             lambda s: len(s) == 3 and s[0] == channels and s[2] == 2
                             and s[1] % 2 == 0 and 2 <= s[1] <= self.MAX_INPUTS)  # fmt: skip
        quad_antennas = _check_array("quad_antennas", quad_antennas, np.int32, "(n_quads, 2)",
                                     lambda s: len(s) == 2 and s[0] >= 1 and s[1] == 2)  # fmt: skip
        n_quads = quad_antennas.shape[0]
        quads = _check_array("quads", quads, np.int32, "(n_quads, 4)",
                             lambda s: s == (n_quads, 4))  # fmt: skip
        if weights is not None:
            weights = _check_array("weights", weights, np.float32, "(channels, baselines)",
                                   lambda s: s == vis.shape)  # fmt: skip
        if flags is not None:
            flags = _check_array("flags", flags, np.uint8, "(channels, baselines)",
                                 lambda s: s == vis.shape)  # fmt: skip
        n_ant = jones.shape[1] // 2
        f32 = np.float32
        t = quads.astype(np.int64)
        present = (t != 0) & (np.abs(t) <= baselines)
        named = np.abs(t[present]) - 1
        counts = np.bincount(named, minlength=1)
        if (counts > 1).any():
            raise ValueError(f"quads names baseline {int(np.argmax(counts > 1))} in more than "
                             f"one entry")  # fmt: skip
        a, b = quad_antennas[:, 0].astype(np.int64), quad_antennas[:, 1].astype(np.int64)
        inr = (a >= 0) & (a < n_ant) & (b >= 0) & (b < n_ant)
        # where each of the four sources comes from: its own entry, or (one dish) its mirror
        source = np.tile(np.arange(4), (n_quads, 1))
        stand = np.zeros((n_quads, 4), bool)
        for entry, other in ((1, 2), (2, 1)):
            stand[:, entry] = (a == b) & ~present[:, entry] & present[:, other]
            source[stand[:, entry], entry] = other
        t_src = np.take_along_axis(t, source, axis=1)
        have = present | stand
        j_src = np.where(have, np.abs(t_src) - 1, 0)
        complete = inr & have.all(axis=1)
        rows_a = 2 * np.where(inr, a, 0)
        rows_b = 2 * np.where(inr, b, 0)
        mul, mul_conj, add = SolveJonesHost._mul, SolveJonesHost._mul_conj, self._add
        with np.errstate(all="ignore"):
            # C_a[i][m], C_b[k][n] as (re, im) pairs of (channels, n_quads)
            ca = [[(jones.real[:, rows_a + i, m], jones.imag[:, rows_a + i, m])
                   for m in range(2)] for i in range(2)]  # fmt: skip
            cb = [[(jones.real[:, rows_b + k, n], jones.imag[:, rows_b + k, n])
                   for n in range(2)] for k in range(2)]  # fmt: skip
            nan = np.zeros((channels, n_quads), bool)
            for matrix in (ca, cb):
                for row in matrix:
                    for re, im in row:
                        nan |= np.isnan(re) | np.isnan(im)
            ok = complete[np.newaxis, :] & ~nan
            s, w = [], []
            for entry in range(4):
                re, im = vis.real[:, j_src[:, entry]], vis.imag[:, j_src[:, entry]]
                im = np.where(t_src[:, entry] < 0, -im, im)
                im = np.where(stand[:, entry], -im, im)
                s.append((re, im))
                if weights is not None:
                    w.append(np.where(have[:, entry], weights[:, j_src[:, entry]], f32(1)))
            # T[i][n], then O[i][k]
            tt = [[add(mul(ca[i][0], s[n]), mul(ca[i][1], s[2 + n])) for n in range(2)]
                  for i in range(2)]  # fmt: skip
            out = [[add(mul_conj(tt[i][0], cb[k][0]), mul_conj(tt[i][1], cb[k][1]))
                    for k in range(2)] for i in range(2)]  # fmt: skip
            assert out[0][0][0].dtype == f32
            out_vis = vis.copy()
            out_weights = None
            if weights is not None:
                out_weights = weights.copy()
                all_w = (w[0] > 0) & (w[1] > 0) & (w[2] > 0) & (w[3] > 0)
                r = [f32(1) / x for x in w]
                norm2 = SolveJonesHost._norm2
                al = [[norm2(ca[i][m]) for m in range(2)] for i in range(2)]
                be = [[norm2(cb[k][n]) for n in range(2)] for k in range(2)]
                u = [[al[i][0] * r[n] + al[i][1] * r[2 + n] for n in range(2)] for i in range(2)]
                var = [[u[i][0] * be[k][0] + u[i][1] * be[k][1] for k in range(2)]
                       for i in range(2)]  # fmt: skip
                assert var[0][0].dtype == f32
            out_flags = None
            if flags is not None:
                out_flags = flags.copy()
                any_f = np.zeros((channels, n_quads), np.uint8)
                for entry in range(4):
                    any_f |= np.where(present[:, entry], flags[:, j_src[:, entry]], np.uint8(0))
                any_f |= np.where(ok, np.uint8(0), np.uint8(self.flag_value))
            for entry in range(4):
                i, k = divmod(entry, 2)
                sel = present[:, entry]
                j = j_src[sel, entry]
                good = ok[:, sel]
                o_re, o_im = out[i][k][0][:, sel], out[i][k][1][:, sel]
                o_im = np.where(t[sel, entry] < 0, -o_im, o_im)
                out_vis.real[:, j] = np.where(good, o_re, vis.real[:, j])
                out_vis.imag[:, j] = np.where(good, o_im, vis.imag[:, j])
                if weights is not None:
                    v = var[i][k][:, sel]
                    scaled = good & all_w[:, sel] & (v > 0)
                    out_weights[:, j] = np.where(scaled, f32(1) / np.where(scaled, v, f32(1)),
                                                 f32(0))  # fmt: skip
                if flags is not None:
                    out_flags[:, j] = any_f[:, sel]
        return out_vis, out_weights, out_flags


class PredictHost:
    """Model visibilities of point sources and, optionally, the data divided by them: the step
    in front of :class:`SolveGainsHost` for a calibrator that is not a unit source at the phase
    centre. ``min sum w |V - g_p conj(g_q) M|^2`` is the unit-model problem on ``V / M`` with
    weights ``w |M|^2``, so the solver takes ``out_vis`` and ``out_weights`` as they are. No
    reference counterpart; this class is the definition that the device operation
    (:class:`.ingest.PredictTemplate`) matches bit for bit.

    ``M[c, j] = sum_s flux[c, s] exp(-2 pi i freqs[c] delays[s, j])``: the caller applies
    spectral index and primary beam to `flux`, and fixes the sign convention through the sign
    of `delays` (:meth:`delays` computes them from ``uvw`` and direction cosines). Per channel
    ``c``, baseline ``j`` and source ``s``, every step one float64 operation, rounded once (a
    multiply, then an add, never an fma)::

        x  = freqs[c] * delays[s, j]                      turns
        r  = x - rint(x)                                  rint: to nearest, ties to even
        q  = rint(4 * r)                                  -2 .. 2
        y  = r - q * 0.25
        z  = y * TWO_PI                                   |z| <= pi/4
        z2 = z * z
        sn = (((((S5*z2 + S4)*z2 + S3)*z2 + S2)*z2 + S1)*z2 + S0) * z       S = SIN_COEFFICIENTS
        cs = (((((C6*z2 + C5)*z2 + C4)*z2 + C3)*z2 + C2)*z2 + C1)*z2 + C0   C = COS_COEFFICIENTS
        (co, si) = (cs, sn), (-sn, cs), (-cs, -sn), (sn, -cs)    for q = 0, 1, +-2, -1
        re = re + float64(flux[c, s]) * co
        im = im - float64(flux[c, s]) * si

    from ``re = im = +0`` with ``s`` ascending; ``model[c, j] = (float32(re), float32(im))``,
    rounded to nearest. A negation flips the sign, so a zero keeps the sign it gets. The
    coefficients are ``(-1)^k / (2k+1)!`` and ``(-1)^k / (2k)!`` as float64; ``(co, si)`` is
    within 7e-12 of the true values, four orders below the float32 rounding of the result.

    With `vis`, every step one float32 operation on the rounded model ``M``::

        d  = M.re*M.re + M.im*M.im
        ok = d > 0 and d < inf                            (false for NaN, underflow, overflow)
        out_vis     = ok ? ((v.re*M.re + v.im*M.im) / d, (v.im*M.re - v.re*M.im) / d) : v
        out_weights = ok ? w * d : 0
        out_flags   = flags | (ok ? 0 : flag_value)

    What follows from it:

    * NaN and infinities go through as IEEE gives them: a non-finite ``x`` gives a NaN model.
    * A sample without a usable model (zero, NaN, or ``d`` under- or overflowing) keeps its
      visibility bit for bit, gets weight 0, "no data" as :class:`SolveGainsHost` reads it, and
      is flagged.

    Parameters
    ----------
    flag_value
        Bits set in ``out_flags`` of a sample without a usable model, 1..255
        (:func:`check_flag_byte`)
    """

    MAX_SOURCES = 64
    SPEED_OF_LIGHT = 299792458.0
    TWO_PI = 6.283185307179586
    #: S0 .. S5
    SIN_COEFFICIENTS = (1.0, -0.16666666666666666, 0.008333333333333333,
                        -0.0001984126984126984, 2.7557319223985893e-06,
                        -2.505210838544172e-08)  # fmt: skip
    #: C0 .. C6
    COS_COEFFICIENTS = (1.0, -0.5, 0.041666666666666664, -0.001388888888888889,
                        2.48015873015873e-05, -2.755731922398589e-07,
                        2.08767569878681e-09)  # fmt: skip

    def __init__(self, flag_value: int = 64) -> None:
        self.flag_value = check_flag_byte("flag_value", flag_value)

    @classmethod
    def delays(cls, uvw, lm) -> np.ndarray:
        """float64 (n_sources, baselines): ``(u l + v m + w (sqrt(1 - l^2 - m^2) - 1)) / c``
        for `uvw` (baselines, 3) in metres and the direction cosines `lm` (n_sources, 2).
        ``ValueError`` for a wrong shape or a source with ``l^2 + m^2 > 1``."""
        uvw = np.asarray(uvw, np.float64)
        lm = np.asarray(lm, np.float64)
        if uvw.ndim != 2 or uvw.shape[1] != 3:
            raise ValueError(f"uvw must have shape (baselines, 3), not {uvw.shape}")
        if lm.ndim != 2 or lm.shape[1] != 2:
            raise ValueError(f"lm must have shape (n_sources, 2), not {lm.shape}")
        l, m = lm[:, 0, np.newaxis], lm[:, 1, np.newaxis]
        n2 = 1.0 - l * l - m * m
        if not (n2 >= 0).all():
            raise ValueError("lm has a source with l^2 + m^2 > 1")
        u, v, w = uvw[np.newaxis, :, 0], uvw[np.newaxis, :, 1], uvw[np.newaxis, :, 2]
        return (u * l + v * m + w * (np.sqrt(n2) - 1.0)) / cls.SPEED_OF_LIGHT

    @classmethod
    def cos_sin(cls, x: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """``(co, si)`` of the class docstring for float64 turns `x`."""
        assert x.dtype == np.float64
        s, c = cls.SIN_COEFFICIENTS, cls.COS_COEFFICIENTS
        with np.errstate(all="ignore"):
            r = x - np.rint(x)
            q = np.rint(4.0 * r)
            y = r - q * 0.25
            z = y * cls.TWO_PI
            z2 = z * z
            sn = s[5]
            for k in (4, 3, 2, 1, 0):
                sn = sn * z2 + s[k]
            sn = sn * z
            cs = c[6]
            for k in (5, 4, 3, 2, 1, 0):
                cs = cs * z2 + c[k]
        odd, half = np.abs(q) == 1.0, np.abs(q) == 2.0
        co = np.where(odd, sn, cs)
        si = np.where(odd, cs, sn)
        co = np.where((q == 1.0) | half, -co, co)
        si = np.where((q == -1.0) | half, -si, si)
        return co, si

    def __call__(self, freqs: np.ndarray, delays: np.ndarray, flux: np.ndarray,
                 vis: Optional[np.ndarray] = None, weights: Optional[np.ndarray] = None,
                 flags: Optional[np.ndarray] = None):  # fmt: skip
        """``(model, out_vis, out_weights, out_flags)``, the last three ``None`` without `vis`
        (and each of the last two without its input), for float64 `freqs` (channels,), float64
        `delays` (n_sources, baselines), float32 `flux` (channels, n_sources), optional
        complex64 `vis`, float32 `weights` and uint8 `flags` (all channels, baselines; the last
        two only with `vis`). ``ValueError``, naming the argument, for a wrong dtype, rank or
        shape (channels and baselines at least 1, n_sources 1..64). No argument is modified."""
        freqs = _check_array("freqs", freqs, np.float64, "(channels,)",
                             lambda s: len(s) == 1 and s[0] >= 1)  # fmt: skip
        channels = freqs.shape[0]
        delays = _check_array("delays", delays, np.float64,
                              "(n_sources, baselines), n_sources 1..64",
                              lambda s: len(s) == 2 and 1 <= s[0] <= self.MAX_SOURCES
                              and s[1] >= 1)  # fmt: skip
        n_sources, baselines = delays.shape
        flux = _check_array("flux", flux, np.float32, "(channels, n_sources)",
                            lambda s: s == (channels, n_sources))  # fmt: skip
        shape = (channels, baselines)
        if vis is not None:
            vis = _check_array("vis", vis, np.complex64, "(channels, baselines)",
                               lambda s: s == shape)  # fmt: skip
        for name, value in (("weights", weights), ("flags", flags)):
            if value is not None and vis is None:
                raise ValueError(f"{name} given without vis")
        if weights is not None:
            weights = _check_array("weights", weights, np.float32, "(channels, baselines)",
                                   lambda s: s == shape)  # fmt: skip
        if flags is not None:
            flags = _check_array("flags", flags, np.uint8, "(channels, baselines)",
                                 lambda s: s == shape)  # fmt: skip
        re = np.zeros(shape, np.float64)
        im = np.zeros(shape, np.float64)
        with np.errstate(all="ignore"):
            for s in range(n_sources):
                co, si = self.cos_sin(freqs[:, np.newaxis] * delays[s][np.newaxis, :])
                amplitude = flux[:, s, np.newaxis].astype(np.float64)
                re = re + amplitude * co
                im = im - amplitude * si
            model = np.empty(shape, np.complex64)
            model.real[...] = re.astype(np.float32)
            model.imag[...] = im.astype(np.float32)
            if vis is None:
                return model, None, None, None
            m_re, m_im = model.real, model.imag
            d = m_re * m_re + m_im * m_im
            ok = (d > 0) & (d < np.inf)
            safe = np.where(ok, d, np.float32(1))  # (the divisor of a sample that stays: no 0 / 0)
            out_vis = np.empty(shape, np.complex64)
            out_vis.real[...] = np.where(ok, (vis.real * m_re + vis.imag * m_im) / safe, vis.real)
            out_vis.imag[...] = np.where(ok, (vis.imag * m_re - vis.real * m_im) / safe, vis.imag)
            assert d.dtype == np.float32 and safe.dtype == np.float32
            out_weights = None
            if weights is not None:
                out_weights = np.where(ok, weights * d, np.float32(0))
        out_flags = None
        if flags is not None:
            out_flags = flags | np.where(ok, np.uint8(0), np.uint8(self.flag_value))
        return model, out_vis, out_weights, out_flags


class FitDelaysHost:
    """Per-input delay (K) fit to the gains that :class:`SolveGainsHost` solves: per input the
    delay and phase whose phasor ``exp(i(phi + 2 pi c channel_width tau))`` best matches the
    gains across the band, and that phasor for every channel of the band, kept or not, which is
    what :class:`ApplyGainsHost` applies. No reference counterpart; this class is the
    definition that the device operation (:class:`.ingest.FitDelaysTemplate`) matches bit for
    bit.

    *Kept channels.* ``x[c] = gains[c, p]`` if both parts are finite and `status` is absent or
    ``status[c] & status_mask == 0``, else 0; channels ``channels .. n_fft-1`` are 0; ``n_kept``
    counts the kept ones. The gains enter with their amplitudes, which is the maximum-likelihood
    weighting for equal noise per channel: they are not normalised.

    *Coarse search*, every step one float32 operation, rounded once (a multiply, then an add,
    never an fma). ``X[k] = sum_c x[c] W^(c k)``, ``W = exp(-2 pi i / n_fft)``, is an in-place
    radix-2 decimation-in-time transform: a bit-reversal permutation, then the stages
    ``s = 1 .. log2 n_fft`` with ``half = 2^(s-1)``, where the butterfly on ``(j, j + half)``
    has the twiddle ``tw = (float32(co), float32(-si))``, ``(co, si) =``
    :meth:`PredictHost.cos_sin` ``((j mod half) / 2^s)``, and::

        bt = (b.re*tw.re - b.im*tw.im, b.re*tw.im + b.im*tw.re);  a' = a + bt;  b' = a - bt

    ``P[k] = re*re + im*im`` and ``k0`` is the lowest ``k`` at which ``P`` takes its largest
    value that is not NaN. There is *no fit* (bit 0 of ``fit_status``) if ``n_kept < 2``, every
    ``P`` is NaN, or that largest value is not in ``(0, inf)``.

    *Refinement*, every step one float64 operation, from ``nu = k0 / n_fft`` turns per channel,
    `refine` times. For each kept channel ``(co, si) = cos_sin(float64(c) * nu)``,
    ``e = (x.re*co + x.im*si, x.im*co - x.re*si)``, and ``D0 = sum e``, ``D1 = sum c*e``,
    ``D2 = sum (c*c)*e``, where every sum is the halving tree over ``Cpad`` terms (the next
    power of two at or above ``channels``; the terms of the other channels are +0):
    ``n = Cpad; while n > 1: n //= 2; t[:n] = t[:n] + t[n:2n]``. Then::

        num  = D1.im*D0.re - D1.re*D0.im
        den  = TWO_PI * ((D1.re*D1.re + D1.im*D1.im) - (D2.re*D0.re + D2.im*D0.im))
        step = num / den
        den < 0 and |step| <= 1/n_fft ?  nu = nu - step  :  set bit 1 and stop

    which is Newton's method on ``|sum x[c] exp(-2 pi i c nu)|^2``, the likelihood of a single
    tone. A NaN fails both tests.

    *Results*, from ``D0`` at the final ``nu``: ``m = sqrt(D0.re*D0.re + D0.im*D0.im)``; no fit
    unless ``m`` is in ``(0, inf)``; ``phasors[p] = (float32(D0.re/m), float32(D0.im/m))``, the
    phase at channel 0; ``amplitudes[p] = float32(m / n_kept)``;
    ``delays[p] = (nu - rint(nu)) / channel_width``; and with ``ph`` the rounded phasor as
    float64 and ``(co, si) = cos_sin(float64(c) * nu)``, ``model[c, p] = (float32(ph.re*co -
    ph.im*si), float32(ph.re*si + ph.im*co))``, the imaginary part negated with `corrections`
    (for a unit modulus the reciprocal). An input without a fit has NaN in ``delays``,
    ``phasors``, ``amplitudes`` and its column of ``model``.

    Parameters
    ----------
    channel_width
        Hz from one channel to the next, finite and not 0; negative for a band stored in
        descending frequency
    n_fft
        Length of the zero-padded transform: a power of two in 4..16384, at least twice the
        channels. ``None``: the smallest power of two at or above four times the channels, at
        most 16384.
    refine
        Newton steps, 0..8
    status_mask
        Bits of `status` that exclude a channel, 0..255 (:func:`check_mask_byte`)
    corrections
        ``True``: ``model`` is the conjugate phasor
    """

    MIN_FFT = 4
    MAX_FFT = 16384
    MAX_CHANNELS = MAX_FFT // 2
    MAX_REFINE = 8
    NO_FIT, STEP_REJECTED = 1, 2
    TWO_PI = PredictHost.TWO_PI

    def __init__(self, channel_width: float, n_fft: Optional[int] = None, refine: int = 3,
                 status_mask: int = 0xFF, corrections: bool = False) -> None:  # fmt: skip
        try:
            width = float(channel_width)
        except (TypeError, ValueError):
            raise ValueError(f"channel_width {channel_width!r} is not a number") from None
        if not np.isfinite(width) or width == 0:
            raise ValueError(f"channel_width {channel_width!r} must be finite and not 0")
        self.channel_width = width
        self.n_fft = None if n_fft is None else self.check_n_fft(n_fft)
        if isinstance(refine, (bool, np.bool_)) or not isinstance(refine, (int, np.integer)):
            raise TypeError(f"refine {refine!r} is not an integer")
        if not 0 <= refine <= self.MAX_REFINE:
            raise ValueError(f"refine must be 0..{self.MAX_REFINE}")
        self.refine = int(refine)
        self.status_mask = check_mask_byte("status_mask", status_mask)
        self.corrections = bool(corrections)

    @classmethod
    def check_n_fft(cls, n_fft) -> int:
        """`n_fft` as an int that is a power of two in 4..16384 (``ValueError`` otherwise,
        ``TypeError`` for a value that is not an integer)."""
        if isinstance(n_fft, (bool, np.bool_)) or not isinstance(n_fft, (int, np.integer)):
            raise TypeError(f"n_fft {n_fft!r} is not an integer")
        if not cls.MIN_FFT <= n_fft <= cls.MAX_FFT or n_fft & (n_fft - 1):
            raise ValueError(f"n_fft must be a power of two in {cls.MIN_FFT}..{cls.MAX_FFT}")
        return int(n_fft)

    def transform_length(self, channels: int, n_inputs: int = 1) -> int:
        """The length of the transform for a band of `channels`: `n_fft`, or its default.
        ``ValueError`` if `channels` is outside 1..8192, `n_inputs` below 1 or `n_fft` below
        twice the channels."""
        if not 1 <= channels <= self.MAX_CHANNELS:
            raise ValueError(f"channels must be 1..{self.MAX_CHANNELS}")
        if n_inputs < 1:
            raise ValueError("n_inputs must be at least 1")
        if self.n_fft is None:
            n_fft = self.MIN_FFT
            while n_fft < 4 * channels and n_fft < self.MAX_FFT:
                n_fft *= 2
            return n_fft
        if self.n_fft < 2 * channels:
            raise ValueError(f"n_fft {self.n_fft} is below twice the channels, {2 * channels}")
        return self.n_fft

    @staticmethod
    def _tree_sum(terms: np.ndarray) -> np.ndarray:
        """The halving tree over the first axis, whose length is a power of two."""
        n = terms.shape[0]
        while n > 1:
            n //= 2
            terms = terms[:n] + terms[n : 2 * n]
        return terms[0]

    @classmethod
    def transform(cls, x_re: np.ndarray, x_im: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """The transform of the class docstring along the first axis of the float32 arrays
        `x_re` and `x_im` (n_fft, ...), as two new arrays."""
        n_fft = x_re.shape[0]
        bits = n_fft.bit_length() - 1
        assert x_re.dtype == np.float32 and x_im.dtype == np.float32 and n_fft == 1 << bits
        index = np.arange(n_fft)
        reverse = np.zeros(n_fft, np.int64)
        for bit in range(bits):
            reverse |= ((index >> bit) & 1) << (bits - 1 - bit)
        rest = x_re.shape[1:]
        re, im = x_re[reverse], x_im[reverse]
        with np.errstate(all="ignore"):
            for s in range(1, bits + 1):
                half = 1 << (s - 1)
                co, si = PredictHost.cos_sin(np.arange(half, dtype=np.float64) / (1 << s))
                shape = (half,) + (1,) * len(rest)
                tw_re = co.astype(np.float32).reshape(shape)
                tw_im = (-si).astype(np.float32).reshape(shape)
                re = re.reshape((-1, 2, half) + rest)
                im = im.reshape((-1, 2, half) + rest)
                a_re, a_im, b_re, b_im = re[:, 0], im[:, 0], re[:, 1], im[:, 1]
                bt_re = b_re * tw_re - b_im * tw_im
                bt_im = b_re * tw_im + b_im * tw_re
                re = np.stack([a_re + bt_re, a_re - bt_re], axis=1)
                im = np.stack([a_im + bt_im, a_im - bt_im], axis=1)
        assert re.dtype == np.float32 and im.dtype == np.float32
        return re.reshape((n_fft,) + rest), im.reshape((n_fft,) + rest)

    def _kept(self, gains: np.ndarray, status: Optional[np.ndarray]) -> np.ndarray:
        kept = np.isfinite(gains.real) & np.isfinite(gains.imag)
        if status is not None:
            kept &= ((status & np.uint8(self.status_mask)) == 0)[:, np.newaxis]
        return kept

    def _sums(self, x_re, x_im, kept, nu):
        """``D0, D1, D2`` as six float64 (n_inputs,) arrays for float64 `x_re`, `x_im`
        (Cpad, n_inputs), zero where not `kept`, at `nu` (n_inputs,)."""
        c = np.arange(x_re.shape[0], dtype=np.float64)[:, np.newaxis]
        co, si = PredictHost.cos_sin(c * nu[np.newaxis, :])
        zero = np.float64(0)
        e_re = np.where(kept, x_re * co + x_im * si, zero)
        e_im = np.where(kept, x_im * co - x_re * si, zero)
        c2 = c * c
        tree = self._tree_sum
        return (tree(e_re), tree(e_im), tree(np.where(kept, c * e_re, zero)),
                tree(np.where(kept, c * e_im, zero)), tree(np.where(kept, c2 * e_re, zero)),
                tree(np.where(kept, c2 * e_im, zero)))  # fmt: skip

    def __call__(self, gains: np.ndarray, status: Optional[np.ndarray] = None):
        """``(delays, phasors, amplitudes, fit_status, model)``: float64, complex64, float32
        and uint8 (n_inputs,) and complex64 (channels, n_inputs), for complex64 `gains`
        (channels, n_inputs) and optional uint8 `status` (channels,). ``ValueError``, naming
        the argument, for a wrong dtype, rank or shape (channels 1..8192, n_inputs at least 1)
        and for an `n_fft` below twice the channels. No argument is modified."""
        gains = _check_array("gains", gains, np.complex64, "(channels, n_inputs)",
                             lambda s: len(s) == 2 and 1 <= s[0] <= self.MAX_CHANNELS
                             and s[1] >= 1)  # fmt: skip
        channels, n_inputs = gains.shape
        if status is not None:
            status = _check_array("status", status, np.uint8, "(channels,)",
                                  lambda s: s == (channels,))  # fmt: skip
        n_fft = self.transform_length(channels, n_inputs)
        f32, f64 = np.float32, np.float64
        kept = self._kept(gains, status)
        n_kept = kept.sum(axis=0)
        x_re = np.zeros((n_fft, n_inputs), f32)
        x_im = np.zeros((n_fft, n_inputs), f32)
        x_re[:channels] = np.where(kept, gains.real, f32(0))
        x_im[:channels] = np.where(kept, gains.imag, f32(0))
        with np.errstate(all="ignore"):
            t_re, t_im = self.transform(x_re, x_im)
            power = t_re * t_re + t_im * t_im
            assert power.dtype == f32
            ranked = np.where(np.isnan(power), f32(-1), power)  # (no power is negative)
            k0 = np.argmax(ranked, axis=0)  # the first of equal values
            peak = ranked[k0, np.arange(n_inputs)]
            no_fit = (n_kept < 2) | ~((peak > 0) & (peak < np.inf))
            fit_status = np.zeros(n_inputs, np.uint8)

            c_pad = 1
            while c_pad < channels:
                c_pad *= 2
            wide_re = np.zeros((c_pad, n_inputs), f64)
            wide_im = np.zeros((c_pad, n_inputs), f64)
            wide_re[:channels] = x_re[:channels]
            wide_im[:channels] = x_im[:channels]
            wide_kept = np.zeros((c_pad, n_inputs), bool)
            wide_kept[:channels] = kept
            nu = k0.astype(f64) / f64(n_fft)
            active = ~no_fit
            for _ in range(self.refine):
                if not active.any():
                    break
                d0r, d0i, d1r, d1i, d2r, d2i = self._sums(wide_re, wide_im, wide_kept, nu)
                num = d1i * d0r - d1r * d0i
                den = self.TWO_PI * ((d1r * d1r + d1i * d1i) - (d2r * d0r + d2i * d0i))
                step = num / den
                accept = (den < 0) & (np.abs(step) <= 1.0 / n_fft)
                nu = np.where(active & accept, nu - step, nu)
                fit_status[active & ~accept] |= np.uint8(self.STEP_REJECTED)
                active = active & accept
            d0r, d0i = self._sums(wide_re, wide_im, wide_kept, nu)[:2]
            m = np.sqrt(d0r * d0r + d0i * d0i)
            no_fit |= ~((m > 0) & (m < np.inf))
            fit_status[no_fit] |= np.uint8(self.NO_FIT)
            safe = np.where(no_fit, f64(1), m)  # (no 0 / 0 where the quotient is not used)
            ph_re = np.where(no_fit, f32(np.nan), (d0r / safe).astype(f32))
            ph_im = np.where(no_fit, f32(np.nan), (d0i / safe).astype(f32))
            amplitudes = np.where(no_fit, f32(np.nan),
                                  (m / np.maximum(n_kept, 1).astype(f64)).astype(f32))  # fmt: skip
            delays = np.where(no_fit, np.nan, (nu - np.rint(nu)) / self.channel_width)
            c = np.arange(channels, dtype=f64)[:, np.newaxis]
            co, si = PredictHost.cos_sin(c * nu[np.newaxis, :])
            wide_ph_re, wide_ph_im = ph_re.astype(f64), ph_im.astype(f64)
            model_re = (wide_ph_re * co - wide_ph_im * si).astype(f32)
            model_im = (wide_ph_re * si + wide_ph_im * co).astype(f32)
            if self.corrections:
                model_im = -model_im
        phasors = np.empty(n_inputs, np.complex64)
        phasors.real[...] = ph_re
        phasors.imag[...] = ph_im
        model = np.empty((channels, n_inputs), np.complex64)
        model.real[...] = np.where(no_fit, f32(np.nan), model_re)
        model.imag[...] = np.where(no_fit, f32(np.nan), model_im)
        assert amplitudes.dtype == f32 and delays.dtype == f64
        return delays, phasors, amplitudes, fit_status, model


class InterpolateGainsHost:
    """The gains that :class:`SolveGainsHost` solves on a calibrator, made into a table that
    :class:`ApplyGainsHost` can apply to a target: per input, the channels the solver left
    without a value (NaN, or excluded by `status`) are filled from their neighbours across gaps
    of at most `max_gap` channels, after the delay that :class:`FitDelaysHost` fitted is divided
    out (linear interpolation of a wound phase loses amplitude) and before it is multiplied
    back in; optionally the bandpass is smoothed, normalised to a mean amplitude of 1,
    multiplied by the band-wide gain of a later solve, and inverted. No reference counterpart;
    this class is the definition that the device operation
    (:class:`.ingest.InterpolateGainsTemplate`) matches bit for bit.

    Every float step is one float32 operation, rounded once (a multiply, then an add, never an
    fma; real and imaginary parts apart; correctly rounded division and square root), as in
    :class:`SolveGainsHost`. A complex product ``a*b`` is ``(a.re*b.re - a.im*b.im, a.re*b.im +
    a.im*b.re)``. Per input ``p``, with ``g = gains[c, p]`` and ``m = model[c, p]``:

    1. *Kept channels.* ``c`` is kept if both parts of ``g`` are finite, `status` is absent or
       ``status[c] & status_mask == 0``, and `model` is absent or both parts of ``m`` are
       finite; every other channel is *missing*. ``kept[p]`` counts the kept ones. If there is
       none, bit 0 of ``fill_status[p]`` (:attr:`NO_DATA`) is set.
    2. *De-rotate.* ``d = g*conj(m) = (g.re*m.re + g.im*m.im, g.im*m.re - g.re*m.im)``, or
       ``d = g`` without `model`.
    3. *Smooth.* For a kept ``c``, ``s[c]`` is the sum of ``d`` over the kept channels of
       ``[c - smooth//2, c + smooth//2]`` that lie inside the band, added one by one in
       ascending channel order from +0, divided by float32 of their number (at least 1: ``c``
       itself). With ``smooth=1`` there is no sum and no division: ``s = d`` bit for bit.
    4. *Normalise* (with `normalise`). ``a`` is the sum of ``sqrt(s.re*s.re + s.im*s.im)`` over
       the kept channels divided by float32 of ``kept[p]``, where the sum is the halving tree
       of :class:`FitDelaysHost` over ``Cpad`` terms (the next power of two at or above
       ``channels``; the terms of the other channels are +0): ``n = Cpad; while n > 1: n //= 2;
       t[:n] = t[:n] + t[n:2n]``. ``mean_amplitude[p] = a``, NaN if no channel is kept. If ``a``
       is in ``(0, inf)``, ``s = (s.re/a, s.im/a)``; otherwise bit 0 is set.
    5. *Fill.* ``y[c] = s[c]`` for a kept ``c``. For a missing ``c`` let ``l`` be the nearest
       kept channel below it and ``r`` the nearest above it. If both exist and ``r - l - 1 <=
       max_gap`` (the gap, whole, is at most `max_gap` channels long), ``t = float32(c - l) /
       float32(r - l)`` and ``y = s[l] + (s[r] - s[l])*t`` per part. If only one exists (``c``
       lies beyond the first or the last kept channel) and ``c`` is at most `max_gap` channels
       away from it, ``y`` is its ``s``: the ends of the band hold the nearest value, channel by
       channel. Otherwise ``y`` is NaN and bit 1 (:attr:`GAP_LEFT`) is set. ``filled[p]``
       counts the missing channels that got a value (whatever IEEE made of it).
    6. *Re-rotate.* With `model`, ``y = y*m`` at every channel, kept or not; a model that is not
       finite gives what IEEE gives. `model` is taken to have unit modulus: its rounding enters
       the amplitude twice, once in each rotation, up to ``2**-22`` relative, which is accepted.
    7. *Scale.* With `scale`, ``y = y*scale[p]``.
    8. *Corrections.* With `corrections` the output is ``(y.re/q, -y.im/q)`` where ``q =
       y.re*y.re + y.im*y.im > 0``, else NaN: what :class:`ApplyGainsHost` multiplies by.

    An input with bit 0 set has NaN in its whole column of ``out``, ``filled[p] = 0`` and no
    other bit. Consequence: with ``smooth=1`` and without `model`, `scale`, `normalise` and
    `corrections`, ``out`` equals ``gains`` bit for bit on every kept channel.

    Parameters
    ----------
    max_gap
        Longest gap that is filled, in channels, 0..16384; 0 fills nothing
    smooth
        Width of the running mean in channels, odd, 1..31
    normalise
        ``True``: divide each input's column by its mean amplitude
    status_mask
        Bits of `status` that make a channel missing, 0..255 (:func:`check_mask_byte`)
    corrections
        ``True``: return the reciprocal gains
    """

    MAX_CHANNELS = 16384
    MAX_GAP = 16384
    MAX_SMOOTH = 31
    NO_DATA, GAP_LEFT = 1, 2

    def __init__(self, max_gap: int, smooth: int = 1, normalise: bool = False,
                 status_mask: int = 0xFF, corrections: bool = False) -> None:  # fmt: skip
        for name, value in (("max_gap", max_gap), ("smooth", smooth)):
            if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
                raise TypeError(f"{name} {value!r} is not an integer")
        if not 0 <= max_gap <= self.MAX_GAP:
            raise ValueError(f"max_gap must be 0..{self.MAX_GAP}")
        if not 1 <= smooth <= self.MAX_SMOOTH or smooth % 2 == 0:
            raise ValueError(f"smooth must be odd and 1..{self.MAX_SMOOTH}")
        self.max_gap = int(max_gap)
        self.smooth = int(smooth)
        self.normalise = bool(normalise)
        self.status_mask = check_mask_byte("status_mask", status_mask)
        self.corrections = bool(corrections)

    @classmethod
    def check_shape(cls, channels: int, n_inputs: int) -> None:
        """``ValueError`` if `channels` is outside 1..16384 or `n_inputs` below 1."""
        if not 1 <= channels <= cls.MAX_CHANNELS:
            raise ValueError(f"channels must be 1..{cls.MAX_CHANNELS}")
        if n_inputs < 1:
            raise ValueError("n_inputs must be at least 1")

    @staticmethod
    def _product(a_re, a_im, b_re, b_im):
        return a_re * b_re - a_im * b_im, a_re * b_im + a_im * b_re

    def __call__(self, gains: np.ndarray, status: Optional[np.ndarray] = None,
                 model: Optional[np.ndarray] = None, scale: Optional[np.ndarray] = None):  # fmt: skip
        """``(out, kept, filled, fill_status, mean_amplitude)``: complex64 (channels, n_inputs),
        int32, int32 and uint8 (n_inputs,), and float32 (n_inputs,) with `normalise`, else
        ``None``; for complex64 `gains` (channels, n_inputs), optional uint8 `status`
        (channels,), optional complex64 `model` (channels, n_inputs) and optional complex64
        `scale` (n_inputs,). ``ValueError``, naming the argument, for a wrong dtype, rank or
        shape (channels 1..16384, n_inputs at least 1). No argument is modified."""
        gains = _check_array("gains", gains, np.complex64, "(channels, n_inputs)",
                             lambda s: len(s) == 2 and 1 <= s[0] <= self.MAX_CHANNELS
                             and s[1] >= 1)  # fmt: skip
        channels, n_inputs = gains.shape
        if status is not None:
            status = _check_array("status", status, np.uint8, "(channels,)",
                                  lambda s: s == (channels,))  # fmt: skip
        if model is not None:
            model = _check_array("model", model, np.complex64, "(channels, n_inputs)",
                                 lambda s: s == gains.shape)  # fmt: skip
        if scale is not None:
            scale = _check_array("scale", scale, np.complex64, "(n_inputs,)",
                                 lambda s: s == (n_inputs,))  # fmt: skip
        f32 = np.float32
        nan, one = f32(np.nan), f32(1)
        kept = np.isfinite(gains.real) & np.isfinite(gains.imag)
        if status is not None:
            kept &= ((status & np.uint8(self.status_mask)) == 0)[:, np.newaxis]
        if model is not None:
            kept &= np.isfinite(model.real) & np.isfinite(model.imag)
        n_kept = kept.sum(axis=0).astype(np.int32)
        failed = n_kept == 0
        mean_amplitude = None
        with np.errstate(all="ignore"):
            s_re, s_im = gains.real, gains.imag
            if model is not None:
                m_re, m_im = model.real, model.imag
                s_re, s_im = s_re * m_re + s_im * m_im, s_im * m_re - s_re * m_im
            if self.smooth > 1:
                reach = self.smooth // 2
                sum_re = np.zeros(gains.shape, f32)
                sum_im = np.zeros(gains.shape, f32)
                count = np.zeros(gains.shape, np.int32)
                for offset in range(-reach, reach + 1):  # channel c + offset, ascending
                    lo, hi = max(0, -offset), min(channels, channels - offset)
                    if lo >= hi:
                        continue
                    to, of = slice(lo, hi), slice(lo + offset, hi + offset)
                    sum_re[to] = np.where(kept[of], sum_re[to] + s_re[of], sum_re[to])
                    sum_im[to] = np.where(kept[of], sum_im[to] + s_im[of], sum_im[to])
                    count[to] += kept[of]
                number = np.maximum(count, 1).astype(f32)  # (only kept channels are used)
                s_re, s_im = sum_re / number, sum_im / number
            if self.normalise:
                c_pad = 1
                while c_pad < channels:
                    c_pad *= 2
                terms = np.zeros((c_pad, n_inputs), f32)
                terms[:channels] = np.where(kept, np.sqrt(s_re * s_re + s_im * s_im), f32(0))
                total = FitDelaysHost._tree_sum(terms)
                mean_amplitude = np.where(failed, nan, total / np.maximum(n_kept, 1).astype(f32))
                usable = (mean_amplitude > 0) & (mean_amplitude < np.inf)
                safe = np.where(usable, mean_amplitude, one)
                s_re, s_im = s_re / safe, s_im / safe
                failed = failed | ~usable
                assert mean_amplitude.dtype == f32
            # the nearest kept channel at or below and at or above every channel
            index = np.arange(channels, dtype=np.int64)[:, np.newaxis]
            none_above = np.int64(channels)
            below = np.maximum.accumulate(np.where(kept, index, -1), axis=0)
            above = np.minimum.accumulate(np.where(kept, index, none_above)[::-1], axis=0)[::-1]
            has_l, has_r = below >= 0, above < none_above
            l, r = np.maximum(below, 0), np.minimum(above, channels - 1)
            sl_re, sl_im = np.take_along_axis(s_re, l, 0), np.take_along_axis(s_im, l, 0)
            sr_re, sr_im = np.take_along_axis(s_re, r, 0), np.take_along_axis(s_im, r, 0)
            span = np.where(has_l & has_r & ~kept, r - l, 1)
            t = (index - l).astype(f32) / span.astype(f32)
            between = has_l & has_r & (above - below - 1 <= self.max_gap)
            held_l = has_l & ~has_r & (index - below <= self.max_gap)
            held_r = has_r & ~has_l & (above - index <= self.max_gap)
            y_re = np.where(between, sl_re + (sr_re - sl_re) * t,
                            np.where(held_l, sl_re, np.where(held_r, sr_re, nan)))  # fmt: skip
            y_im = np.where(between, sl_im + (sr_im - sl_im) * t,
                            np.where(held_l, sl_im, np.where(held_r, sr_im, nan)))  # fmt: skip
            y_re, y_im = np.where(kept, s_re, y_re), np.where(kept, s_im, y_im)
            got = ~kept & (between | held_l | held_r)
            if model is not None:
                y_re, y_im = self._product(y_re, y_im, m_re, m_im)
            if scale is not None:
                y_re, y_im = self._product(y_re, y_im, scale.real[np.newaxis, :],
                                           scale.imag[np.newaxis, :])  # fmt: skip
            if self.corrections:
                q = y_re * y_re + y_im * y_im
                pos = q > 0
                safe = np.where(pos, q, one)  # (no 0 / 0 where the quotient is not used)
                y_re = np.where(pos, y_re / safe, nan)
                y_im = np.where(pos, -y_im / safe, nan)
            assert y_re.dtype == f32 and y_im.dtype == f32
        out = np.empty(gains.shape, np.complex64)
        out.real[...] = np.where(failed, nan, y_re)
        out.imag[...] = np.where(failed, nan, y_im)
        filled = np.where(failed, 0, got.sum(axis=0)).astype(np.int32)
        fill_status = np.where(failed, self.NO_DATA,
                               np.where((~kept & ~got).any(axis=0), self.GAP_LEFT, 0)
                               ).astype(np.uint8)  # fmt: skip
        return out, n_kept, filled, fill_status, mean_amplitude


class InterpolateJonesHost(InterpolateGainsHost):
    """The 2x2 counterpart of :class:`InterpolateGainsHost`: the matrices that
    :class:`SolveJonesHost` solves on a calibrator (``corrections=False``), made into a table
    that :class:`ApplyJonesHost` can apply to a target. Per antenna, the channels the solver
    left without a matrix are filled from their neighbours across gaps of at most `max_gap`
    channels; a matrix is interpolated whole or not at all. No reference counterpart; this
    class is the definition that the device operation
    (:class:`.ingest.InterpolateJonesTemplate`) matches bit for bit.

    The parameters, their checks, :attr:`NO_DATA` and :attr:`GAP_LEFT` are those of
    :class:`InterpolateGainsHost`, and so is the arithmetic: one float32 operation per step,
    rounded once, real and imaginary parts apart, the complex products as written there and in
    :class:`SolveJonesHost`. ``jones[c, 2a + i, k]`` is element ``(i, k)`` of antenna ``a``'s
    matrix. Per antenna ``a``, with ``z[i][k] = jones[c, 2a + i, k]`` and ``m_i = model[c, 2a +
    i]`` (one unit phasor per feed, what :class:`FitDelaysHost` fits to the diagonal that
    :class:`JonesDiagonalHost` extracts):

    1. *Kept channels.* ``c`` is kept if all eight floats of the matrix are finite, `status` is
       absent or ``status[c] & status_mask == 0``, and `model` is absent or all four floats of
       ``m_0``, ``m_1`` are finite. One mask per antenna. ``kept[a]`` counts the kept channels;
       none sets bit 0.
    2. *De-rotate.* ``d[i][k] = z[i][k]*conj(m_i)`` (step 2 there), ``d = z`` without `model`.
       After the solver's referencing, element ``(i, k)`` winds with the delay of feed ``i`` of
       ``a`` minus that of feed ``k`` of the reference antenna; the per-row model removes all
       of it from the diagonal and leaves the reference antenna's own cross-feed delay on the
       leakage terms.
    3. *Smooth.* Per element, step 3 there; the four elements share the count.
    4. *Normalise* (with `normalise`). Per kept channel ``term = sqrt(((n00 + n01) + (n10 +
       n11))*0.5)`` with ``nik = s.re*s.re + s.im*s.im`` of element ``(i, k)``; ``a`` is the
       halving tree of the terms over ``Cpad`` divided by float32 of ``kept[a]``, as there;
       ``mean_amplitude[a] = a``, NaN with nothing kept. If ``a`` is in ``(0, inf)`` all eight
       floats are divided by it, otherwise bit 0 is set. An identity matrix has amplitude 1.
    5. *Fill.* Per element, step 5 there, with the same ``l``, ``r`` and ``t`` for the four
       elements. ``filled[a]`` counts the missing channels that got a matrix.
    6. *Re-rotate.* ``y[i][k] = y[i][k]*m_i`` at every channel.
    7. *Scale.* ``y[i][k] = y[i][k]*scale[2a + i]``.
    8. *Corrections.* As in :class:`SolveJonesHost`: with ``[[a, b], [c, d]] = y``, ``D = a*d -
       b*c``, ``s = D.re*D.re + D.im*D.im``, ``inv = (D.re/s, -D.im/s)`` and the matrix becomes
       ``[[d*inv, -(b*inv)], [-(c*inv), a*inv]]`` (the products are negated, not the factor);
       all four elements are NaN unless ``s > 0``.

    An antenna with bit 0 has NaN in all its elements of ``out``, ``filled[a] = 0`` and no
    other bit. With ``smooth=1`` and without `model`, `scale`, `normalise` and `corrections`,
    ``out`` equals ``jones`` bit for bit on every kept channel. On exactly diagonal matrices
    whose two feeds have the same kept channels, and without `corrections` and `normalise` (the
    amplitude of a matrix is not that of one of its elements), the diagonal of ``out`` is
    :class:`InterpolateGainsHost`'s ``out`` for those inputs bit for bit and the off-diagonals
    stay zero.
    """

    MAX_INPUTS = ApplyJonesHost.MAX_INPUTS

    @classmethod
    def check_shape(cls, channels: int, n_inputs: int) -> None:
        """``ValueError`` if `channels` is outside 1..16384 or `n_inputs` is odd or outside
        2..2048."""
        if not 1 <= channels <= cls.MAX_CHANNELS:
            raise ValueError(f"channels must be 1..{cls.MAX_CHANNELS}")
        ApplyJonesHost.check_n_inputs(n_inputs)

    def __call__(self, jones: np.ndarray, status: Optional[np.ndarray] = None,
                 model: Optional[np.ndarray] = None, scale: Optional[np.ndarray] = None):  # fmt: skip
        """``(out, kept, filled, fill_status, mean_amplitude)``: complex64 (channels, n_inputs,
        2), int32, int32 and uint8 (n_inputs // 2,), and float32 (n_inputs // 2,) with
        `normalise`, else ``None``; for complex64 `jones` (channels, n_inputs, 2), optional
        uint8 `status` (channels,), optional complex64 `model` (channels, n_inputs) and
        optional complex64 `scale` (n_inputs,). ``ValueError``, naming the argument, for a
        wrong dtype, rank or shape (channels 1..16384, n_inputs even and 2..2048). No argument
        is modified."""
        jones = _check_array("jones", jones, np.complex64, "(channels, n_inputs, 2)",
                             lambda s: len(s) == 3 and 1 <= s[0] <= self.MAX_CHANNELS
                             and s[1] % 2 == 0 and 2 <= s[1] <= self.MAX_INPUTS
                             and s[2] == 2)  # fmt: skip
        channels, n_inputs = jones.shape[:2]
        n_ant = n_inputs // 2
        if status is not None:
            status = _check_array("status", status, np.uint8, "(channels,)",
                                  lambda s: s == (channels,))  # fmt: skip
        if model is not None:
            model = _check_array("model", model, np.complex64, "(channels, n_inputs)",
                                 lambda s: s == (channels, n_inputs))  # fmt: skip
        if scale is not None:
            scale = _check_array("scale", scale, np.complex64, "(n_inputs,)",
                                 lambda s: s == (n_inputs,))  # fmt: skip
        f32 = np.float32
        nan, one = f32(np.nan), f32(1)
        # element e = 2 i + k of every antenna, (channels, n_ant) per part; row i has model i
        z = [(jones.real[:, i::2, k], jones.imag[:, i::2, k]) for i in (0, 1) for k in (0, 1)]
        kept = np.ones((channels, n_ant), bool)
        for re, im in z:
            kept &= np.isfinite(re) & np.isfinite(im)
        if status is not None:
            kept &= ((status & np.uint8(self.status_mask)) == 0)[:, np.newaxis]
        m = None
        if model is not None:
            m = [(model.real[:, i::2], model.imag[:, i::2]) for i in (0, 1)]
            for re, im in m:
                kept &= np.isfinite(re) & np.isfinite(im)
        n_kept = kept.sum(axis=0).astype(np.int32)
        failed = n_kept == 0
        mean_amplitude = None
        with np.errstate(all="ignore"):
            s = z
            if m is not None:
                s = [(re * m[e // 2][0] + im * m[e // 2][1], im * m[e // 2][0] - re * m[e // 2][1])
                     for e, (re, im) in enumerate(s)]  # fmt: skip
            if self.smooth > 1:
                reach = self.smooth // 2
                sums = [[np.zeros(kept.shape, f32), np.zeros(kept.shape, f32)] for _ in s]
                count = np.zeros(kept.shape, np.int32)
                for offset in range(-reach, reach + 1):  # channel c + offset, ascending
                    lo, hi = max(0, -offset), min(channels, channels - offset)
                    if lo >= hi:
                        continue
                    to, of = slice(lo, hi), slice(lo + offset, hi + offset)
                    for total, parts in zip(sums, s):
                        for i in range(2):
                            total[i][to] = np.where(kept[of], total[i][to] + parts[i][of],
                                                    total[i][to])  # fmt: skip
                    count[to] += kept[of]
                number = np.maximum(count, 1).astype(f32)  # (only kept channels are used)
                s = [(total[0] / number, total[1] / number) for total in sums]
            if self.normalise:
                c_pad = 1
                while c_pad < channels:
                    c_pad *= 2
                n2 = [re * re + im * im for re, im in s]
                terms = np.zeros((c_pad, n_ant), f32)
                terms[:channels] = np.where(
                    kept, np.sqrt(((n2[0] + n2[1]) + (n2[2] + n2[3])) * f32(0.5)), f32(0))
                total = FitDelaysHost._tree_sum(terms)
                mean_amplitude = np.where(failed, nan, total / np.maximum(n_kept, 1).astype(f32))
                usable = (mean_amplitude > 0) & (mean_amplitude < np.inf)
                safe = np.where(usable, mean_amplitude, one)
                s = [(re / safe, im / safe) for re, im in s]
                failed = failed | ~usable
                assert mean_amplitude.dtype == f32
            # the nearest kept channel at or below and at or above every channel
            index = np.arange(channels, dtype=np.int64)[:, np.newaxis]
            none_above = np.int64(channels)
            below = np.maximum.accumulate(np.where(kept, index, -1), axis=0)
            above = np.minimum.accumulate(np.where(kept, index, none_above)[::-1], axis=0)[::-1]
            has_l, has_r = below >= 0, above < none_above
            l, r = np.maximum(below, 0), np.minimum(above, channels - 1)
            span = np.where(has_l & has_r & ~kept, r - l, 1)
            t = (index - l).astype(f32) / span.astype(f32)
            between = has_l & has_r & (above - below - 1 <= self.max_gap)
            held_l = has_l & ~has_r & (index - below <= self.max_gap)
            held_r = has_r & ~has_l & (above - index <= self.max_gap)
            got = ~kept & (between | held_l | held_r)
            y = []
            for e, parts in enumerate(s):
                filled_parts = []
                for part in parts:
                    sl, sr = np.take_along_axis(part, l, 0), np.take_along_axis(part, r, 0)
                    value = np.where(between, sl + (sr - sl) * t,
                                     np.where(held_l, sl, np.where(held_r, sr, nan)))  # fmt: skip
                    filled_parts.append(np.where(kept, part, value))
                y_re, y_im = filled_parts
                if m is not None:
                    y_re, y_im = self._product(y_re, y_im, m[e // 2][0], m[e // 2][1])
                if scale is not None:
                    y_re, y_im = self._product(y_re, y_im, scale.real[np.newaxis, e // 2 :: 2],
                                               scale.imag[np.newaxis, e // 2 :: 2])  # fmt: skip
                y.append((y_re, y_im))
            if self.corrections:
                ja, jb, jc, jd = y
                ad, bc = self._product(*ja, *jd), self._product(*jb, *jc)
                big_d = (ad[0] - bc[0], ad[1] - bc[1])
                q = big_d[0] * big_d[0] + big_d[1] * big_d[1]
                pos = q > 0
                safe = np.where(pos, q, one)  # (no 0 / 0 where the quotient is not used)
                inv = (big_d[0] / safe, -big_d[1] / safe)
                di, bi = self._product(*jd, *inv), self._product(*jb, *inv)
                ci, ai = self._product(*jc, *inv), self._product(*ja, *inv)
                y = [tuple(np.where(pos, part, nan) for part in parts)
                     for parts in (di, (-bi[0], -bi[1]), (-ci[0], -ci[1]), ai)]  # fmt: skip
            assert all(part.dtype == f32 for parts in y for part in parts)
        out = np.empty(jones.shape, np.complex64)
        for e, (y_re, y_im) in enumerate(y):
            out.real[:, e // 2 :: 2, e % 2] = np.where(failed, nan, y_re)
            out.imag[:, e // 2 :: 2, e % 2] = np.where(failed, nan, y_im)
        filled = np.where(failed, 0, got.sum(axis=0)).astype(np.int32)
        fill_status = np.where(failed, self.NO_DATA,
                               np.where((~kept & ~got).any(axis=0), self.GAP_LEFT, 0)
                               ).astype(np.uint8)  # fmt: skip
        return out, n_kept, filled, fill_status, mean_amplitude


class JonesDiagonalHost:
    """The diagonal of every antenna's matrix as per-input gains: ``gains[c, p] = jones[c, p,
    p % 2]``, a copy of bits. It is what :class:`FitDelaysHost` reads to fit one delay per feed
    to the table of :class:`SolveJonesHost` (after whose referencing the reference antenna's
    diagonal is real and positive, so that its fitted phasor is 1 and the delays of all feeds
    are defined against it); the `model` it writes is the one :class:`InterpolateJonesHost`
    takes. The device operation is :class:`.ingest.JonesDiagonalTemplate`."""

    def __call__(self, jones: np.ndarray) -> np.ndarray:
        """complex64 (channels, n_inputs) for complex64 `jones` (channels, n_inputs, 2) with
        at least one channel and one input; ``ValueError`` otherwise."""
        jones = _check_array("jones", jones, np.complex64, "(channels, n_inputs, 2)",
                             lambda s: len(s) == 3 and s[0] >= 1 and s[1] >= 1
                             and s[2] == 2)  # fmt: skip
        n_inputs = jones.shape[1]
        gains = np.empty(jones.shape[:2], np.complex64)
        gains.view(np.uint64)[...] = np.ascontiguousarray(jones).view(np.uint64)[
            :, np.arange(n_inputs), np.arange(n_inputs) % 2]  # fmt: skip
        return gains


def check_ranges(ranges, baselines: Optional[int] = None) -> Tuple[Tuple[int, int], ...]:
    """`ranges` as a tuple of 1 to :attr:`RangePercentilesHost.MAX_RANGES` pairs of ints
    ``(start, stop)`` with ``0 <= start <= stop``, ``stop - start`` at most
    :attr:`RangePercentilesHost.MAX_LENGTH` and, if `baselines` is given, ``stop <= baselines``
    (``ValueError`` naming ``ranges`` otherwise)."""
    try:
        pairs = [tuple(pair) for pair in ranges]
    except TypeError:
        raise ValueError(f"ranges {ranges!r} is not a sequence of (start, stop) pairs") from None
    if not 1 <= len(pairs) <= RangePercentilesHost.MAX_RANGES:
        raise ValueError(f"ranges must hold 1..{RangePercentilesHost.MAX_RANGES} pairs, "
                         f"not {len(pairs)}")  # fmt: skip
    checked = []
    for pair in pairs:
        if len(pair) != 2 or any(isinstance(v, (bool, np.bool_))
                                 or not isinstance(v, (int, np.integer)) for v in pair):  # fmt: skip
            raise ValueError(f"ranges: {pair!r} is not a pair of integers (start, stop)")
        start, stop = int(pair[0]), int(pair[1])
        if not 0 <= start <= stop:
            raise ValueError(f"ranges: ({start}, {stop}) does not satisfy 0 <= start <= stop")
        if stop - start > RangePercentilesHost.MAX_LENGTH:
            raise ValueError(f"ranges: ({start}, {stop}) is longer than "
                             f"{RangePercentilesHost.MAX_LENGTH} columns")  # fmt: skip
        if baselines is not None and stop > baselines:
            raise ValueError(f"ranges: ({start}, {stop}) ends beyond the {baselines} baselines")
        checked.append((start, stop))
    return tuple(checked)


def check_mask_byte(name: str, value) -> int:
    """`value` as an int in 0..255 (``ValueError`` otherwise, ``TypeError`` for a value that
    is not an integer)."""
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)):
        raise TypeError(f"{name} {value!r} is not an integer")
    if not 0 <= value <= 255:
        raise ValueError(f"{name} {value} is outside 0..255")
    return int(value)


class RangePercentilesHost:
    """The signal-display product of a dump: for every range of baselines (a group such as
    "auto HH") and every channel, the 0/100/25/75/50 % amplitudes of the samples that carry
    data, how many those are, and the OR of the group's flags. No reference counterpart; this
    class is the definition that the device operation
    (:class:`.ingest.RangePercentilesTemplate`) matches bit for bit. For channel ``c`` and
    range ``(start, stop)`` number ``r``::

        a[b]   = data[c, b] if float32, numpy.abs(data[c, b]) if complex64   (b in [start, stop))
        kept   = { b : not isnan(a[b]) and (flags[c, b] & mask) == 0 }  (no flags: no second term)
        K      = sort(a[kept]);  n = len(K)
        counts[r, c]         = n
        percentiles[r, :, c] = K[0], K[n-1], K[(n-1)//4], K[3*(n-1)//4], K[(n-1)//2]
                               (five +0.0 when n == 0)
        range_flags[r, c]    = OR of flags[c, b] over ALL b in [start, stop)  (0 if there are none)

    The indices are those of ``numpy.percentile(K, [0, 100, 25, 75, 50], method="lower")``,
    and the row order is that of the reference's ``Percentile5``; with nothing left out the
    five rows of a range are what ``Percentile5`` gives for that ``column_range``.

    Why samples are left out: a flagged sample is interference the flagger already found, and
    a display whose "max" and "75 %" lines follow it hides the band underneath; a NaN is what
    :class:`AveragerHost` never produces but a caller's own averaging may leave where there was
    no data, and it must not count as "larger than everything". ``range_flags`` still reports
    every flag of the group, kept or not.

    float32 `data` must be non-negative with the sign bit clear, or NaN (the restriction of
    ``Percentile5``, whose rank search the device shares). This class sorts whatever it is
    given; the device gives an unspecified value in the percentiles of a range that holds a
    negative value or ``-0.0`` (never an access outside the arrays). ``+inf`` is an ordinary
    largest value.

    Parameters
    ----------
    ranges
        1 to 16 pairs ``(start, stop)``; they may be empty, overlap, repeat and come in any
        order; at most 16384 columns each (:func:`check_ranges`)
    mask
        0..255: a sample with ``flags & mask != 0`` is left out; 0 leaves out NaN alone
    """

    MAX_RANGES = 16
    MAX_LENGTH = 16384

    def __init__(self, ranges, mask: int = 0) -> None:
        self.ranges = check_ranges(ranges)
        self.mask = check_mask_byte("mask", mask)

    def __call__(self, data: np.ndarray, flags: Optional[np.ndarray] = None):
        """``(percentiles, counts, range_flags)``: float32 (n_ranges, 5, channels), uint32
        (n_ranges, channels) and uint8 (n_ranges, channels) -- ``None`` without `flags` -- for
        float32 or complex64 `data` (channels, baselines), both at least 1, and optional uint8
        `flags` of the same shape. ``TypeError`` for a non-zero mask without `flags`;
        ``ValueError``, naming the argument, for a wrong dtype, rank or shape or a range that
        ends beyond the baselines."""
        data = np.asarray(data)
        dtype = np.complex64 if data.dtype == np.complex64 else np.float32
        data = _check_array("data", data, dtype, "(channels, baselines)",
                            lambda s: len(s) == 2 and s[0] >= 1 and s[1] >= 1)  # fmt: skip
        channels, baselines = data.shape
        if flags is None:
            if self.mask != 0:
                raise TypeError(f"mask {self.mask:#x} was given but flags were not provided")
        else:
            flags = _check_array("flags", flags, np.uint8, "(channels, baselines)",
                                 lambda s: s == data.shape)  # fmt: skip
        check_ranges(self.ranges, baselines)
        n_ranges = len(self.ranges)
        percentiles = np.zeros((n_ranges, 5, channels), np.float32)
        counts = np.zeros((n_ranges, channels), np.uint32)
        range_flags = None if flags is None else np.zeros((n_ranges, channels), np.uint8)
        rows = np.arange(channels)
        for r, (start, stop) in enumerate(self.ranges):
            if start == stop:
                continue
            with np.errstate(all="ignore"):
                a = np.abs(data[:, start:stop]) if dtype == np.complex64 else data[:, start:stop]
            assert a.dtype == np.float32
            kept = ~np.isnan(a)
            if flags is not None:
                part = flags[:, start:stop]
                kept &= (part & np.uint8(self.mask)) == 0
                range_flags[r] = np.bitwise_or.reduce(part, axis=1)
            n = kept.sum(axis=1)
            counts[r] = n
            # (NaN sorts last: the kept values are the first n of a sorted row)
            ordered = np.sort(np.where(kept, a, np.float32(np.nan)), axis=1)
            last = np.maximum(n - 1, 0)
            for k, index in enumerate((0 * last, last, last // 4, 3 * last // 4, last // 2)):
                percentiles[r, k] = np.where(n > 0, ordered[rows, index], np.float32(0))
        return percentiles, counts, range_flags


class BandAverageHost:
    """The other signal-display product of a dump, the "time series": for every baseline and
    each of up to :attr:`MAX_SERIES` series of channel weights (a sub-band each, say), the
    weighted mean of the visibility and of its amplitude over the channels that carry data,
    the weight sum, how many samples were kept and the OR of the series' flags. No reference
    counterpart; this class is the definition that the device operation
    (:class:`.ingest.BandAverageTemplate`) matches bit for bit. For series ``k`` and baseline
    ``b``, every step one float32 operation, rounded once, in this order::

        w      = channel_weights[k, c]
        in_k   = w > 0             (a zero, negative or NaN weight leaves channel c out of series k)
        kept   = in_k and not isnan(re) and not isnan(im) and (flags[c, b] & mask) == 0
                                   (no flags: no last term)
        a      = numpy.abs(data[c, b])

        for each block j of BLOCK consecutive channels (the last may be short), from +0.0:
            for c ascending in the block, if kept:
                p_re += w * re;  p_im += w * im;  p_a += w * a;  p_w += w
                (a multiply, then an add: never an fma)
        S_re, S_im, S_a, S_w = the block partials added in ascending j, from +0.0

        counts[k, b]         = number of kept samples
        series_flags[k, b]   = OR of flags[c, b] over ALL c with in_k, kept or not
        weight_sums[k, b]    = S_w
        mean[k, b]           = (S_re / S_w, S_im / S_w) if S_w > 0 else (0, 0)
        mean_amplitude[k, b] = S_a / S_w if S_w > 0 else 0

    Infinities and denormals go through as IEEE arithmetic gives them; a NaN sum makes
    ``S_w > 0`` false only if it is the weight sum. A sample that is not kept adds nothing
    (which, as every sum starts at +0.0, is the same as adding +0.0). Where a result is NaN
    (``inf - inf``, ``inf / inf``) it is NaN on the device too; its sign and payload are the
    processor's.

    Why samples are left out: as for :class:`RangePercentilesHost`; and once they are, the
    kept set differs from baseline to baseline, so the normaliser has to come from the same
    pass. Why blocks: the device splits the reduction over channels to fill the chip, so the
    order of the sums has to be fixed here and not by a launch geometry. :attr:`BLOCK` is
    part of the arithmetic, not a tuning value.

    Parameters
    ----------
    mask
        0..255: a sample with ``flags & mask != 0`` is left out; 0 leaves out NaN alone
        (:func:`check_mask_byte`)
    """

    BLOCK = 128
    MAX_SERIES = 8
    MAX_CHANNELS = 262144

    def __init__(self, mask: int = 0) -> None:
        self.mask = check_mask_byte("mask", mask)

    def __call__(self, data: np.ndarray, channel_weights: np.ndarray,
                 flags: Optional[np.ndarray] = None):  # fmt: skip
        """``(mean, mean_amplitude, weight_sums, counts, series_flags)``: complex64, float32,
        float32, uint32 and uint8 -- ``None`` without `flags` --, each (n_series, baselines),
        for complex64 `data` (channels, baselines), both at least 1 and channels at most
        262144, float32 `channel_weights` (n_series, channels) with 1 to 8 series, and
        optional uint8 `flags` of `data`'s shape. ``TypeError`` for a non-zero mask without
        `flags`; ``ValueError``, naming the argument, for a wrong dtype, rank or shape."""
        data = _check_array("data", data, np.complex64, "(channels <= 262144, baselines)",
                            lambda s: len(s) == 2 and 1 <= s[0] <= self.MAX_CHANNELS and s[1] >= 1)  # fmt: skip
        channels, baselines = data.shape
        channel_weights = _check_array(
            "channel_weights", channel_weights, np.float32, "(1..8 series, channels)",
            lambda s: len(s) == 2 and 1 <= s[0] <= self.MAX_SERIES and s[1] == channels)  # fmt: skip
        if flags is None:
            if self.mask != 0:
                raise TypeError(f"mask {self.mask:#x} was given but flags were not provided")
        else:
            flags = _check_array("flags", flags, np.uint8, "(channels, baselines)",
                                 lambda s: s == data.shape)  # fmt: skip
        n_series = channel_weights.shape[0]
        block = self.BLOCK
        n_blocks = -(-channels // block)
        padded = n_blocks * block
        zero = np.float32(0)
        with np.errstate(all="ignore"):
            amplitude = np.abs(data)
        assert amplitude.dtype == np.float32
        ok = ~(np.isnan(data.real) | np.isnan(data.imag))
        if flags is not None:
            ok &= (flags & np.uint8(self.mask)) == 0

        def blocks(values, fill):
            """(channels, ...) as (n_blocks, BLOCK, ...), the short last block filled up."""
            out = np.full((padded,) + values.shape[1:], fill, values.dtype)
            out[:channels] = values
            return out.reshape((n_blocks, block) + values.shape[1:])

        parts = [blocks(np.ascontiguousarray(v), zero) for v in (data.real, data.imag, amplitude)]
        ok_blocks = blocks(ok, False)
        sums = np.zeros((4, n_series, baselines), np.float32)
        counts = np.zeros((n_series, baselines), np.uint32)
        series_flags = None if flags is None else np.zeros((n_series, baselines), np.uint8)
        for k in range(n_series):
            with np.errstate(invalid="ignore"):
                in_k = channel_weights[k] > 0
            w_blocks = blocks(np.where(in_k, channel_weights[k], zero), zero)
            in_blocks = blocks(in_k, False)
            partial = np.zeros((4, n_blocks, baselines), np.float32)
            for i in range(min(block, channels)):  # the position inside a block, all blocks at once
                kept = ok_blocks[:, i] & in_blocks[:, i, np.newaxis]
                w = w_blocks[:, i, np.newaxis]
                with np.errstate(all="ignore"):
                    for t in range(3):
                        partial[t] += np.where(kept, w * parts[t][:, i], zero)
                    partial[3] += np.where(kept, w, zero)
                counts[k] += kept.sum(axis=0, dtype=np.uint32)
            with np.errstate(all="ignore"):
                for j in range(n_blocks):
                    sums[:, k] += partial[:, j]
            if flags is not None and in_k.any():
                series_flags[k] = np.bitwise_or.reduce(flags[in_k], axis=0)
        s_w = sums[3]
        with np.errstate(invalid="ignore"):
            some = s_w > 0
        divisor = np.where(some, s_w, np.float32(1))  # (no division where there is no result)
        with np.errstate(all="ignore"):
            mean = np.zeros((n_series, baselines), np.complex64)
            mean.real[...] = np.where(some, sums[0] / divisor, zero)
            mean.imag[...] = np.where(some, sums[1] / divisor, zero)
            mean_amplitude = np.where(some, sums[2] / divisor, zero)
        assert partial.dtype == np.float32 and mean_amplitude.dtype == np.float32
        return mean, mean_amplitude, s_w.copy(), counts, series_flags


class FlaggerHost(AbstractFlaggerHost):
    """background -> noise estimate -> threshold (reference rfi/host.py:257-273)."""

    def __init__(self, background: AbstractBackgroundHost, noise_est: AbstractNoiseEstHost,
                 threshold: AbstractThresholdHost) -> None:  # fmt: skip
        self.background = background
        self.noise_est = noise_est
        self.threshold = threshold

    def __call__(self, vis: np.ndarray, input_flags: Optional[np.ndarray] = None) -> np.ndarray:
        deviations = self.background(vis, input_flags)
        return self.threshold(deviations, self.noise_est(deviations))
