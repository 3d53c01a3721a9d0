#!/usr/bin/env python3
"""Generate ``rfi_host_nonfinite_golden.npz``: infinite (and NaN) input from the REAL
reference, in the manner of ``make_golden.py``.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONPATH=<reference>/src python3 tests/golden/make_golden_nonfinite.py

The reference's background is ``pd.DataFrame(amp).rolling(width, center=True,
min_periods=1).median()``; pandas turns +-inf into NaN before the rolling median, so an
infinite sample takes no part in any window, while the deviation ``amp - med`` uses the
raw amplitude (``inf - median = inf``; ``inf - NaN = NaN``, which ``fillna(0)`` makes 0).
These vectors pin that behaviour. Inputs come from the seeded generators
``tests.inputs.nonfinite_*``:

* ``nonfinite_case`` (complex, 4096 x 12): background deviations and the full flagger
  (MAD, SumThreshold with 4 windows, 11 sigma) for widths 5, 13, 31, 63 and 255 x flag
  modes none / channel / full;
* ``nonfinite_amp_case`` (amplitudes, 1024 x 5, with +-inf and negatives): the same;
* ``nonfinite_mad_case`` (float32 deviations) at 4096, 4097, 20000 and 20001 channels:
  ``NoiseEstMADHost``;
* ``nonfinite_threshold_case`` (float32 deviations and noise): ``ThresholdSimpleHost`` and
  ``ThresholdSumHost`` with 1 to 8 windows.

Deviations are stored as a sha256 of their float64 bytes plus, for mode "none", the rows
``inputs.nonfinite_rows()`` around the planted samples; flags as packed bits. The archive
is written with fixed member timestamps, so that a rerun reproduces it byte for byte.

Versions used for the committed fixture: numpy 2.2.6, pandas 2.3.3, Python 3.10.12.
"""

import hashlib
import io
import os
import sys
import warnings
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

from katsdpsigproc.rfi import host  # noqa: E402  (the reference)

from tests import inputs  # noqa: E402  (seeded input generators shared with the tests)

WIDTHS = inputs.NONFINITE_WIDTHS
MAD_CHANNELS = inputs.NONFINITE_MAD_CHANNELS


def digest(a: np.ndarray) -> str:
    a = np.ascontiguousarray(a)
    if a.dtype.kind == "f":
        a = a + 0.0  # normalise -0.0
    return hashlib.sha256(a.tobytes()).hexdigest()


def main() -> None:
    out = {}
    # (the all-inf baselines give numpy's "Mean of empty slice": their noise is NaN)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for tag in ("cplx", "amp"):
            vis, in_flags, amplitudes, rows, chan_col = inputs.nonfinite_input(tag)
            for width in WIDTHS:
                bg = host.BackgroundMedianFilterHost(width, amplitudes)
                flagger = host.FlaggerHost(bg, host.NoiseEstMADHost(), host.ThresholdSumHost(11.0))
                for mode, fl in (("none", None), ("channel", in_flags[:, chan_col]),
                                 ("full", in_flags)):  # fmt: skip
                    key = f"{tag}_w{width}_{mode}"
                    dev = bg(vis) if fl is None else bg(vis, fl)
                    assert dev.dtype == np.float64
                    out[key + "_dev_sha"] = np.array(digest(dev))
                    if mode == "none":
                        out[key + "_dev_rows"] = dev[rows]
                    out[key + "_noise"] = host.NoiseEstMADHost()(dev)
                    flags = flagger(vis) if fl is None else flagger(vis, fl)
                    out[key + "_flags"] = np.packbits(flags.astype(np.bool_))

        for channels in MAD_CHANNELS:
            out[f"mad_{channels}"] = host.NoiseEstMADHost()(inputs.nonfinite_mad_case(channels))

        dev, noise = inputs.nonfinite_threshold_case()
        out["threshold_simple"] = np.packbits(host.ThresholdSimpleHost(11.0)(dev, noise).astype(np.bool_))
        for n_windows in range(1, 9):
            fl = host.ThresholdSumHost(11.0, n_windows=n_windows)(dev, noise)
            out[f"threshold_sum_w{n_windows}"] = np.packbits(fl.astype(np.bool_))

    out["versions"] = np.array(f"numpy {np.__version__}, pandas {host.pd.__version__}")
    path = inputs.NONFINITE_GOLDEN
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
