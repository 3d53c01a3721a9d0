"""Seeded inputs for the tests of ``rfi.host.ApplyGainsHost`` and of the device operation
(tests/test_apply_gains.py, tests/test_gpu_apply_gains.py), and the comparison both use."""

import numpy as np

f32 = np.float32
INT32_MIN, INT32_MAX = -(2**31), 2**31 - 1
TINY = f32(2.0**-149)  # the smallest denormal

#: index patterns of :func:`make_inputs`
PATTERNS = ("random", "one", "stride32", "auto", "outside")
#: what :func:`make_gains` sprinkles over the ordinary gains, about 2 % of the elements each
SPECIAL_GAINS = (
    complex(np.nan, 1.0),  # NaN in the real part only
    complex(1.0, np.nan),  # NaN in the imaginary part only
    complex(np.inf, 0.5),
    complex(0.5, -np.inf),
    complex(-np.inf, np.inf),
    complex(0.0, 0.0),
    complex(-0.0, 0.0),
    complex(float(TINY) * 3, -float(TINY)),  # denormals
    complex(2.0**-130, 2.0**-140),
    complex(1e-30, 1e-30),  # p underflows to 0
    complex(1e30, -1e30),  # p overflows to +inf
)


def make_gains(seed, channels, n_inputs, special=True):
    """complex64 (channels, n_inputs): magnitudes 2^U(-20, 20) with a random phase and, with
    `special`, each of SPECIAL_GAINS in about 2 % of the elements."""
    rs = np.random.RandomState(seed)
    shape = (channels, n_inputs)
    magnitude = np.exp2(rs.uniform(-20, 20, shape))
    phase = rs.uniform(0, 2 * np.pi, shape)
    gains = (magnitude * np.exp(1j * phase)).astype(np.complex64)
    if special:
        kind = rs.random_sample(shape)
        for i, value in enumerate(SPECIAL_GAINS):
            gains[(kind >= 0.02 * i) & (kind < 0.02 * (i + 1))] = value
    return gains


def make_inputs(seed, pattern, baselines, n_inputs):
    """int32 (baselines, 2). ``random``: any pair; ``one``: every entry the same input (every
    LDS read of a wavefront is a broadcast); ``stride32``: neighbouring baselines 32 inputs
    apart (gains 256 bytes apart: every lane of a group on one bank); ``auto``: a == b;
    ``outside``: random pairs of which about a quarter have -1, n_inputs, INT32_MIN or
    INT32_MAX on one side or both."""
    rs = np.random.RandomState(seed)
    j = np.arange(baselines)
    if pattern == "random":
        inputs = rs.randint(0, n_inputs, (baselines, 2))
    elif pattern == "one":
        inputs = np.full((baselines, 2), rs.randint(n_inputs))
    elif pattern == "stride32":
        inputs = np.stack([(32 * j) % n_inputs, (32 * j + 32 * (j // 7)) % n_inputs], axis=1)
    elif pattern == "auto":
        inputs = np.repeat(rs.randint(0, n_inputs, (baselines, 1)), 2, axis=1)
    elif pattern == "outside":
        inputs = rs.randint(0, n_inputs, (baselines, 2)).astype(np.int64)
        bad = np.array([-1, n_inputs, INT32_MIN, INT32_MAX], np.int64)
        side = rs.randint(0, 8, baselines)  # 0: a, 1: b, 2: both, 3..7: neither
        which = bad[(j + rs.randint(4)) % 4]
        inputs[:, 0] = np.where((side == 0) | (side == 2), which, inputs[:, 0])
        inputs[:, 1] = np.where((side == 1) | (side == 2), which[::-1], inputs[:, 1])
    else:
        raise ValueError(pattern)
    return np.ascontiguousarray(inputs, np.int32)


def make_vis(seed, channels, baselines):
    """complex64 (channels, baselines): normal deviates times 2^U(-10, 10), with +-0, NaN and
    infinities in about 1 % of the parts each."""
    rs = np.random.RandomState(seed)
    shape = (channels, baselines)
    vis = np.empty(shape, np.complex64)
    for part in (vis.real, vis.imag):
        part[...] = rs.standard_normal(shape) * np.exp2(rs.uniform(-10, 10, shape))
        kind = rs.random_sample(shape)
        for i, value in enumerate([0.0, -0.0, np.nan, np.inf, -np.inf]):
            part[(kind >= 0.01 * i) & (kind < 0.01 * (i + 1))] = value
    return vis


def make_weights(seed, channels, baselines):
    """float32 (channels, baselines): 2^U(-10, 10) with 0, 2^30 and 2^-30 in about 3 % each."""
    rs = np.random.RandomState(seed)
    shape = (channels, baselines)
    weights = np.exp2(rs.uniform(-10, 10, shape)).astype(f32)
    kind = rs.random_sample(shape)
    for i, value in enumerate([0.0, 2.0**30, 2.0**-30]):
        weights[(kind >= 0.03 * i) & (kind < 0.03 * (i + 1))] = value
    return weights


def make_flags(seed, channels, baselines, flag_value=128):
    """uint8 (channels, baselines): half zero, the rest random bytes, and about 10 % with
    `flag_value` already set."""
    rs = np.random.RandomState(seed)
    shape = (channels, baselines)
    flags = rs.randint(0, 256, shape).astype(np.uint8)
    flags[rs.random_sample(shape) < 0.5] = 0
    flags[rs.random_sample(shape) < 0.1] |= np.uint8(flag_value)
    return flags


def make_case(seed, channels, baselines, n_inputs, pattern="random", flag_value=128):
    """dict of vis, gains, inputs, weights, flags for one shape."""
    return {
        "vis": make_vis(seed, channels, baselines),
        "gains": make_gains(seed + 1, channels, n_inputs),
        "inputs": make_inputs(seed + 2, pattern, baselines, n_inputs),
        "weights": make_weights(seed + 3, channels, baselines),
        "flags": make_flags(seed + 4, channels, baselines, flag_value),
    }


def assert_same(want, got, what=""):
    """Same dtype, shape and bit patterns; the one exception is a float (or a part of a
    complex number) that is NaN in `want`, which has to be a NaN in `got`."""
    assert want.dtype == got.dtype and want.shape == got.shape, what
    want, got = np.ascontiguousarray(want), np.ascontiguousarray(got)
    if want.dtype == np.uint8:
        bad = want != got
        words_want, words_got = want, got
    else:
        parts_want, parts_got = want.view(f32), got.view(f32)
        words_want, words_got = want.view(np.uint32), got.view(np.uint32)
        nan = np.isnan(parts_want)
        bad = np.where(nan, ~np.isnan(parts_got), words_want != words_got)
    assert not bad.any(), (
        f"{what}: {np.count_nonzero(bad)} of {bad.size} words differ, first at "
        f"{np.argwhere(bad)[0]}: want {words_want[bad][0]:#x}, got {words_got[bad][0]:#x}")  # fmt: skip
