"""NumPy restatement of ``masked_gaussian_filter`` (reference rfi/twodflag.py:254-400) for
float32 and float64 images and any number of box passes.

Test infrastructure: it imports only NumPy. The arithmetic is DESIGN.md section 9's: every
line carries the reference's float64 running sum in the reference's order, every pass is
stored in the line's type, the divisor is numba's ``d ** passes`` by squaring in that type.
Each pass reads only the previous pass's values, so its running sum is one sequential
``np.cumsum`` of the interleaved terms (+new, -old, +new, ...); the lines are vectorised.
"""

import numpy as np

#: lines per block of the box filter (bounds the float64 temporaries)
_BOX_LANES = 2048


def radius(sigma, passes):
    return int(0.5 * np.sqrt(12.0 * np.float64(sigma) ** 2 / passes + 1))


def divisor(r, passes, dtype):
    """numba's ``dtype(2 r + 1) ** passes`` (``int_power_impl``)."""
    scalar = np.dtype(dtype).type
    result, base, e = scalar(1), scalar(2 * r + 1), int(passes)
    with np.errstate(over="ignore"):  # (the last squaring is not used)
        while e:
            if e & 1:
                result = scalar(result * base)
            base = scalar(base * base)
            e >>= 1
    return result


def box_sums(lines, r, passes):
    """The box passes of one line per row, padded by r * passes zeros on the left."""
    lanes, n = lines.shape
    pad, r2 = r * passes, 2 * r
    L = n + pad
    P = np.zeros((lanes, L), lines.dtype)
    P[:, pad:] = lines
    prev_start = pad
    for p in range(1, passes + 1):
        start = pad - r2 * p
        stop = start + n + 2 * pad
        start, stop = max(start, 0), min(stop, L)
        tail = min(stop, L - r2)
        if tail < start:
            raise ValueError("one pass with a box radius beyond the line")
        head = P[:, prev_start:min(start + r2, L)]
        k0, na, nb = head.shape[1], tail - start, stop - tail
        terms = np.empty((lanes, k0 + 2 * na + nb), np.float64)
        terms[:, :k0] = head
        terms[:, k0:k0 + 2 * na:2] = P[:, start + r2:tail + r2]
        terms[:, k0 + 1:k0 + 2 * na:2] = -P[:, start:tail].astype(np.float64)
        terms[:, k0 + 2 * na:] = -P[:, tail:stop].astype(np.float64)
        # run[:, j] = s before term j is added (s starts from 0.0)
        run = np.cumsum(np.concatenate([np.zeros((lanes, 1)), terms], axis=1), axis=1)
        P[:, start:tail] = run[:, k0 + 1:k0 + 2 * na + 1:2]
        P[:, tail:stop] = run[:, k0 + 2 * na:k0 + 2 * na + nb]
        prev_start = start
    return P[:, :n]


def box_filter(lines, r, passes):
    """Box filter of every row (r > 0), divided by numba's d ** passes."""
    out = np.empty_like(lines)
    div = divisor(r, passes, lines.dtype)
    for i in range(0, lines.shape[0], _BOX_LANES):
        out[i:i + _BOX_LANES] = box_sums(lines[i:i + _BOX_LANES], r, passes) / div
    return out


def smooth(img, r0, r1, passes):
    """``_box_gaussian_filter`` of (B, rows, cols) images: along axis 0, then along axis 1."""
    B, R, C = img.shape
    if r0 > 0:
        lines = np.ascontiguousarray(img.transpose(0, 2, 1)).reshape(B * C, R)
        img = box_filter(lines, r0, passes).reshape(B, C, R).transpose(0, 2, 1)
    if r1 > 0:
        img = box_filter(np.ascontiguousarray(img).reshape(B * R, C), r1, passes).reshape(B, R, C)
    return np.ascontiguousarray(img)


def masked_filter(data, flags, sigma, passes=4):
    """``masked_gaussian_filter`` of a 2-D image or a stack of them; returns the result."""
    dtype = data.dtype
    assert dtype in (np.float32, np.float64) and data.shape == flags.shape
    img = data.reshape((-1,) + data.shape[-2:])
    flagged = flags.reshape(img.shape) != 0
    r0, r1 = radius(sigma[0], passes), radius(sigma[1], passes)
    weight = smooth(np.where(flagged, dtype.type(0), dtype.type(1)), r0, r1, passes)
    out = smooth(np.where(flagged, dtype.type(0), img), r0, r1, passes)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        out = np.where(weight == 0, dtype.type(np.nan), out / weight).astype(dtype)
    return out.reshape(data.shape)
