#!/usr/bin/env python3
"""Generate ``rfi_host_nan_deviations_golden.npz``: the noise estimate of the REAL reference on
NaN deviations, in the manner of ``make_golden_nonfinite.py`` (whose archive stays as it is).

Run in the build container only (the reference never travels to the GPU box):

    PYTHONPATH=<reference>/src python3 tests/golden/make_golden_nan_deviations.py

``mad_nan_<channels>`` is the reference's ``NoiseEstMADHost`` (``np.median(abs_dev[abs_dev >
0]) * 1.4826`` per baseline, float64) on ``tests.inputs_nan_deviations.nan_mad_case(channels,
67)`` at 4096, 4097, 20000 and 20001 channels, the lengths of ``mad_<channels>`` in the other
archive. The archive is written with fixed member timestamps, so that a rerun reproduces it byte
for byte.

Versions used for the committed fixture: numpy 2.2.6, Python 3.10.12.
"""

import io
import os
import sys
import warnings
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

from katsdpsigproc.rfi import host  # noqa: E402  (the reference)

from tests import inputs_nan_deviations as nd  # noqa: E402  (seeded input generators)


def main() -> None:
    out = {}
    # (columns with nothing left give numpy's "Mean of empty slice": their noise is NaN)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for channels in nd.GOLDEN_CHANNELS:
            dev = nd.nan_mad_case(channels, nd.MAD_COLUMNS)
            out[f"mad_nan_{channels}"] = host.NoiseEstMADHost()(dev)
    out["versions"] = np.array(f"numpy {np.__version__}")
    with zipfile.ZipFile(nd.GOLDEN, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())
    print("wrote", nd.GOLDEN, os.path.getsize(nd.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
