#!/usr/bin/env python3
"""Generate ``rfi_host_long_golden.npz``: the noise estimate and the flagger on bands
longer than 16384 channels, from the REAL reference, in the manner of ``make_golden.py``.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONPATH=/root/reference/src python3 tests/golden/make_golden_long.py

It runs the reference's ``katsdpsigproc.rfi.host`` (src/katsdpsigproc/rfi/host.py) on
seeded inputs from ``tests/inputs_long.py``:

* ``NoiseEstMADHost`` on float32 deviations of 32768 x 8 and 262144 x 2 (standard
  normal, about 10 % zeros), stored as float64;
* ``FlaggerHost(BackgroundMedianFilterHost(13), NoiseEstMADHost(), ThresholdSumHost(11.0))``
  on a 32768 x 16 RFI case, without and with per-sample input flags, stored as packed
  bits.

Versions used for the committed fixtures: numpy 2.2.6, pandas 2.3.3, Python 3.10.12.
"""

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

from katsdpsigproc.rfi import host  # noqa: E402  (the reference)

from tests import inputs_long  # noqa: E402  (seeded input generators shared with the tests)

NOISE_SHAPES = ((32768, 8), (262144, 2))


def main() -> None:
    out = {}
    for channels, baselines in NOISE_SHAPES:
        dev = inputs_long.noise_long_case(channels, baselines)
        out[f"noise_{channels}x{baselines}"] = host.NoiseEstMADHost()(dev)

    vis, in_flags = inputs_long.flagger_long_case()
    flagger = host.FlaggerHost(
        host.BackgroundMedianFilterHost(13), host.NoiseEstMADHost(), host.ThresholdSumHost(11.0)
    )
    out["flagger_32768_none"] = np.packbits(flagger(vis).astype(np.bool_))
    out["flagger_32768_full"] = np.packbits(flagger(vis, in_flags).astype(np.bool_))

    path = os.path.join(HERE, "rfi_host_long_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
