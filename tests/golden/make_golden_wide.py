#!/usr/bin/env python3
"""Generate ``rfi_host_wide_golden.npz``: wide median windows (odd widths 33 to 255) from
the REAL reference, in the manner of ``make_golden.py``.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONPATH=/root/reference/src python3 tests/golden/make_golden_wide.py

It runs the reference's ``katsdpsigproc.rfi.host`` (src/katsdpsigproc/rfi/host.py) on
seeded inputs from ``tests/inputs.py``, all finite:

* ``BackgroundMedianFilterHost(width)`` for width in 33, 63, 127, 255 x {complex,
  amplitude} x {no flags, channel flags, per-sample flags} on the 417 x 313 background
  case of the reference's test (test/rfi/test_background.py:33-45);
* width 255 on the first 100 channels of that case (a band narrower than the window);
* one ``FlaggerHost`` with width 63 and SumThreshold on the flagger case
  (test/rfi/test_flagger.py:36-52), with and without per-sample input flags.

Deviations are stored as a sha256 of their float64 bytes plus the columns
``inputs.BACKGROUND_COLS``; flags as packed bits.

Versions used for the committed fixtures: numpy 2.2.6, pandas 2.3.3, Python 3.10.12.
"""

import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

from katsdpsigproc.rfi import host  # noqa: E402  (the reference)

from tests import inputs  # noqa: E402  (seeded input generators shared with the tests)

WIDTHS = (33, 63, 127, 255)


def digest(a: np.ndarray) -> str:
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        a = a + 0.0  # normalise -0.0
    return hashlib.sha256(a.tobytes()).hexdigest()


def store(out, key, dev):
    assert dev.dtype == np.float64
    out[key + "_sha"] = np.array(digest(dev))
    out[key + "_cols"] = dev[:, inputs.BACKGROUND_COLS]


def main() -> None:
    out = {}
    vis_big, flags_big = inputs.background_case()
    for width in WIDTHS:
        for amplitudes in (False, True):
            vis = np.abs(vis_big) if amplitudes else vis_big
            bg = host.BackgroundMedianFilterHost(width, amplitudes)
            for mode, flags in (("none", None), ("channel", flags_big[:, 0]), ("full", flags_big)):
                dev = bg(vis) if flags is None else bg(vis, flags)
                store(out, f"background_w{width}_{'amp' if amplitudes else 'cplx'}_{mode}", dev)

    # a band of 100 channels under a window of 255
    narrow = vis_big[:100]
    store(out, "background_w255_narrow_cplx_full",
          host.BackgroundMedianFilterHost(255)(narrow, flags_big[:100]))

    vis_f, _spikes, in_flags = inputs.flagger_case()
    flagger = host.FlaggerHost(
        host.BackgroundMedianFilterHost(63), host.NoiseEstMADHost(), host.ThresholdSumHost(11.0)
    )
    out["flagger_w63_sum_none"] = np.packbits(flagger(vis_f).astype(np.bool_))
    out["flagger_w63_sum_full"] = np.packbits(flagger(vis_f, in_flags).astype(np.bool_))

    path = os.path.join(HERE, "rfi_host_wide_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
