#!/usr/bin/env python3
"""Generate ``rfi_host_threshold_edges_golden.npz``: the REAL reference's flags for the inputs
of ``tests.inputs_threshold_edges`` -- window sums and samples on their limit, where float32
deviations decide wrongly -- in the manner of ``make_golden_nonfinite.py``.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONPATH=<reference>/src python3 tests/golden/make_golden_threshold_edges.py

Every case of at most 4096 channels goes through the reference's ``FlaggerHost`` (pandas rolling
median, ``NoiseEstMADHost``, ``ThresholdSumHost`` or ``ThresholdSimpleHost``) with the case's
width, flag mode, ``n_sigma``, ``n_windows`` and ``threshold_falloff``. Stored per case: the
sha256 of the flag bytes and their count, and for the 320-channel cases the flags themselves as
packed bits. The archive is written with fixed member timestamps, so that a rerun reproduces it
byte for byte.

Versions used for the committed fixture: numpy 2.2.6, pandas 2.3.3, Python 3.10.12.
"""

import hashlib
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

from katsdpsigproc.rfi import host  # noqa: E402  (the reference)

from tests import inputs_threshold_edges as edges  # noqa: E402


def main() -> None:
    out = {}
    for case in edges.all_cases():
        if case.vis.shape[0] > edges.GOLDEN_MAX_CHANNELS:
            continue
        bg = host.BackgroundMedianFilterHost(case.width, case.amplitudes)
        if case.kind == "simple":
            thr = host.ThresholdSimpleHost(case.n_sigma)
        else:
            thr = host.ThresholdSumHost(case.n_sigma, n_windows=case.n_windows,
                                        threshold_falloff=case.threshold_falloff)  # fmt: skip
        flagger = host.FlaggerHost(bg, host.NoiseEstMADHost(), thr)
        flags = flagger(case.vis) if case.in_flags is None else flagger(case.vis, case.in_flags)
        flags = np.ascontiguousarray(flags, np.uint8)
        out[case.name + "_sha"] = np.array(hashlib.sha256(flags.tobytes()).hexdigest())
        out[case.name + "_count"] = np.array(int(np.count_nonzero(flags)))
        if case.vis.shape[0] <= edges.GOLDEN_PACKED_CHANNELS:
            out[case.name + "_flags"] = np.packbits(flags.astype(np.bool_))
    out["versions"] = np.array(f"numpy {np.__version__}, pandas {host.pd.__version__}")
    path = edges.GOLDEN
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
