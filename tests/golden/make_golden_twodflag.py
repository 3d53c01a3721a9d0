#!/usr/bin/env python3
"""Generate ``rfi_twodflag_golden.npz``: flags of the REAL reference
``katsdpsigproc.rfi.twodflag.SumThresholdFlagger`` for the cases of
``tests/inputs_twodflag.py``.

The reference is numba code. It runs as plain Python when the stub ``numba`` module below
is imported first (``jit`` returns the function, ``extending.overload`` a no-op
decorator). Run in the build container only (the reference never travels to the GPU box):

    PYTHONPATH=<reference>/src python3 tests/golden/make_golden_twodflag.py

Three adjustments make plain NumPy 2 compute what the numba-compiled reference computes
(DESIGN.md section 9 lists the typing points):

* ``average_freq``, ``time_extend`` and ``freq_extend`` become int64 0-d arrays after
  construction (uint8 ones overflow in ``n_freq + factor - 1`` under NumPy 2; values
  unchanged);
* ``outlier_nsigma`` and ``background_reject`` are passed as ``np.float64``, so that the
  threshold multiplies happen in float64 as numba types them;
* ``_linearly_interpolate_nans1d`` is replaced by a version with a float64 gradient and
  float64 interpolated values (numba: float32 / int64 -> float64), and ``_average_freq``
  by one that takes ``np.abs`` of the whole block (the project's |z|, NumPy's vectorised
  complex64 abs) and adds each group's channels in channel order in float32, as the
  reference's loop does.

Flags are stored packed (``np.packbits``); for ``inputs.STAGE_CASE`` the per-baseline 2-D
background (float32) and time flags (packed) are stored too. The archive has fixed member
timestamps, so that a rerun reproduces it byte for byte.
"""

import io
import json
import os
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))


def _install_numba_stub():
    numba = types.ModuleType("numba")

    def jit(*args, **kwargs):
        if args and callable(args[0]):
            return args[0]
        return lambda f: f

    numba.jit = jit
    numba.extending = types.SimpleNamespace(overload=lambda *a, **k: (lambda f: f))
    numba.types = types.SimpleNamespace(
        Boolean=type("Boolean", (), {}), Integer=type("Integer", (), {})
    )
    sys.modules["numba"] = numba


_install_numba_stub()

from katsdpsigproc.rfi import twodflag  # noqa: E402  (the reference)

from tests import inputs_twodflag as inputs  # noqa: E402


def _interpolate_nans_f64(data):
    """Fill NaNs of a 1-D float32 row: end values repeated outwards, straight lines
    between valid neighbours with the gradient and the sums in float64."""
    valid = np.flatnonzero(~np.isnan(data))
    if valid.size == 0:
        data[:] = 0
        return
    data[: valid[0]] = data[valid[0]]
    data[valid[-1] + 1:] = data[valid[-1]]
    for left, right in zip(valid[:-1], valid[1:]):
        if right - left > 1:
            start = data[left]
            grad = np.float64(data[right] - start) / np.int64(right - left)
            for i in range(left + 1, right):
                data[i] = np.float64(start) + np.int64(i - left) * grad


def _average_freq_vectorised(in_data, in_flags, factor):
    if in_data.shape != in_flags.shape:
        raise ValueError("shape mismatch")
    n_time, n_freq, n_bl = in_data.shape
    factor = int(factor)
    a_freq = (n_freq + factor - 1) // factor
    amp = np.abs(in_data).astype(np.float32)
    valid = ~(in_flags.astype(np.bool_)) & ~np.isnan(amp)
    total = np.zeros((n_time, a_freq, n_bl), np.float32)
    weight = np.zeros((n_time, a_freq, n_bl), np.int64)
    for k in range(factor):
        ch = np.arange(k, n_freq, factor)
        rows = ch // factor
        total[:, rows] += np.where(valid[:, ch], amp[:, ch], np.float32(0))
        weight[:, rows] += valid[:, ch]
    flags = weight == 0
    avg = np.where(flags, np.float32(0), total / np.maximum(weight, 1).astype(np.float32))
    return (np.ascontiguousarray(avg.transpose(2, 0, 1)).astype(np.float32),
            np.ascontiguousarray(flags.transpose(2, 0, 1)))  # fmt: skip


twodflag._linearly_interpolate_nans1d = _interpolate_nans_f64
twodflag._average_freq = _average_freq_vectorised


def reference_flagger(params):
    kw = dict(params)
    kw["outlier_nsigma"] = np.float64(kw.get("outlier_nsigma", 4.5))
    kw["background_reject"] = np.float64(kw.get("background_reject", 2.0))
    flagger = twodflag.SumThresholdFlagger(**kw)
    for name in ("average_freq", "time_extend", "freq_extend"):
        setattr(flagger, name, np.array(int(getattr(flagger, name)), np.int64))
    return flagger


def main() -> None:
    out = {"cases": np.array(json.dumps(inputs.case_list(), sort_keys=True))}
    for case in inputs.case_list():
        name = case["name"]
        data, flags = inputs.make_case(name)
        stages = {"background": [], "time_flags": []}
        if name == inputs.STAGE_CASE:
            bg2d, st = twodflag._get_background2d, twodflag._sum_threshold

            def spy_bg(data_, *args):
                result = bg2d(data_, *args)
                if data_.shape[0] > 1:
                    stages["background"].append(result.copy())
                return result

            def spy_st(data_, flags_, axis, *args):
                result = st(data_, flags_, axis, *args)
                if axis == 0:
                    stages["time_flags"].append(result.copy())
                return result

            twodflag._get_background2d, twodflag._sum_threshold = spy_bg, spy_st
        try:
            result = reference_flagger(case["params"]).get_flags(data, flags)
        finally:
            if name == inputs.STAGE_CASE:
                twodflag._get_background2d, twodflag._sum_threshold = bg2d, st
        out[f"{name}_flags"] = np.packbits(result.astype(np.bool_))
        if name == inputs.STAGE_CASE:
            out[f"{name}_background"] = np.stack(stages["background"]).astype(np.float32)
            out[f"{name}_time_flags"] = np.packbits(np.stack(stages["time_flags"]))
        print(name, data.shape, int(result.sum()), "flags", flush=True)
    out["versions"] = np.array(f"numpy {np.__version__}")
    with zipfile.ZipFile(inputs.GOLDEN, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())
    print("wrote", inputs.GOLDEN, os.path.getsize(inputs.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
