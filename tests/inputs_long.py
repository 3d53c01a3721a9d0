"""Seeded inputs for bands beyond 16384 channels, shared by ``golden/make_golden_long.py``
and the tests that check against its fixture."""

import numpy as np

from tests import inputs


def noise_long_case(channels, baselines, seed=21, zeros=0.1):
    """Channel-major float32 deviations, standard normal with a fraction `zeros` set to 0."""
    rs = np.random.RandomState(seed=seed)
    dev = rs.standard_normal((channels, baselines)).astype(np.float32)
    dev[rs.random_sample((channels, baselines)) < zeros] = 0.0
    return dev


def flagger_long_case(channels=32768, baselines=16):
    """Noise with RFI on 1/16 of the samples and per-sample input flags (1/16, value 2)."""
    vis = inputs.add_rfi(inputs.generate_data(channels, baselines, seed=5), seed=6)
    rs = np.random.RandomState(seed=7)
    flags = (rs.random_sample((channels, baselines)) < 1.0 / 16.0).astype(np.uint8) * 2
    return vis, flags
