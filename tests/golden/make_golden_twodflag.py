#!/usr/bin/env python3
"""Generate ``rfi_twodflag_golden.npz``: flags of the REAL reference
``katsdpsigproc.rfi.twodflag.SumThresholdFlagger`` for the cases of
``tests/inputs_twodflag.py``.

The reference is numba code. It runs as plain Python when the stub ``numba`` module below
is imported first (``jit`` returns the function, ``extending.overload`` a no-op
decorator). Run in the build container only (the reference never travels to the GPU box):

    PYTHONPATH=<reference>/src python3 tests/golden/make_golden_twodflag.py

Four adjustments make plain NumPy 2 compute what the numba-compiled reference computes
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
  reference's loop does;
* ``_box_gaussian_filter1d`` gets its ``passes`` as an int whose ``float32 ** passes`` is
  numba's ``int_power_impl``, squaring in float32. NumPy's float32 power rounds d ** 4
  differently once d >= 65 (69 ** 4: 22667122 against numba's 22667120).

Flags are stored packed (``np.packbits``); for ``inputs.STAGE_CASE`` the per-baseline 2-D
background (float32) and time flags (packed) are stored too. For ``inputs.STAGE_CASES``
``rfi_twodflag_stages_golden.npz`` holds every stage of ``inputs.RECORDED_STAGES``, recorded
per baseline in call order by spies on the reference's functions (float32 as they are,
flags packed). The archives have fixed member timestamps, so that a rerun reproduces them
byte for byte.

``--check-oracle N`` instead runs N seeded random small parameter sets through both the
reference and ``oracle/twodflag_oracle.py`` and reports every stage that differs.
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


class _NumbaPasses(int):
    """An int whose power of a float32 is numba's: repeated squaring in float32."""

    __array_ufunc__ = None  # NumPy scalars defer to __rpow__

    def __rpow__(self, base):
        result, base, e = np.float32(1), np.float32(base), int(self)
        while e:
            if e & 1:
                result = np.float32(result * base)
            base = np.float32(base * base)
            e >>= 1
        return result

    def __rmul__(self, other):  # r * passes with a NumPy integer r
        return other * int(self)


def _with_numba_power(box1d):
    def wrapper(data, r, out, passes):
        return box1d(data, r, out, _NumbaPasses(passes))

    return wrapper


twodflag._linearly_interpolate_nans1d = _interpolate_nans_f64
twodflag._average_freq = _average_freq_vectorised
twodflag._box_gaussian_filter1d = _with_numba_power(twodflag._box_gaussian_filter1d)


def reference_flagger(params):
    kw = dict(params)
    kw["outlier_nsigma"] = np.float64(kw.get("outlier_nsigma", 4.5))
    kw["background_reject"] = np.float64(kw.get("background_reject", 2.0))
    flagger = twodflag.SumThresholdFlagger(**kw)
    for name in ("average_freq", "time_extend", "freq_extend"):
        setattr(flagger, name, np.array(int(getattr(flagger, name)), np.int64))
    return flagger


class _Spies:
    """Records the reference's stages per baseline, in call order, while installed."""

    NAMES = ("_time_median", "_get_background2d", "_sum_threshold", "_combine_flags",
             "_unaverage_freq")  # fmt: skip

    def __init__(self):
        self.stages = {name: [] for name in inputs.RECORDED_STAGES}
        self.orig = {name: getattr(twodflag, name) for name in self.NAMES}
        self.n_bg = self.n_st = 0

    def _time_median(self, data, flags):
        result = self.orig["_time_median"](data, flags)
        self.stages["spec_flags"].append(result[1][0].copy())
        return result

    def _get_background2d(self, data, flags, *args):
        result = self.orig["_get_background2d"](data, flags, *args)
        # per baseline: the spectrum's, then the 2-D one
        key = "background" if self.n_bg % 2 else "spec_background"
        self.stages[key].append(result[0].copy() if key == "spec_background" else result.copy())
        self.n_bg += 1
        return result

    def _sum_threshold(self, data, flags, axis, *args):
        result = self.orig["_sum_threshold"](data, flags, axis, *args)
        step = self.n_st % 3  # spectrum, time, frequency
        if step == 0:
            self.stages["spec_residual"].append(data[0].copy())
            self.stages["spec_st"].append(result[0].copy())
        elif step == 1:
            self.stages["residual"].append(data.copy())
            self.stages["flags"].append(flags.copy())
            self.stages["time_flags"].append(result.copy())
        else:
            self.stages["freq_flags"].append(result.copy())
        self.n_st += 1
        return result

    def _combine_flags(self, spec, time_flags, freq_flags, time_extend, out):
        self.orig["_combine_flags"](spec, time_flags, freq_flags, time_extend, out)
        self.stages["combined"].append(out.copy())

    def _unaverage_freq(self, flags, freq_extend, average_freq, frac_time, frac_freq, out):
        # the smeared row flags alone: the same call without whole rows and columns
        rows = np.zeros_like(out)
        self.orig["_unaverage_freq"](flags, freq_extend, average_freq, np.inf, np.inf, rows)
        self.stages["row_flags"].append(rows.copy())
        self.orig["_unaverage_freq"](flags, freq_extend, average_freq, frac_time, frac_freq, out)
        self.stages["unaveraged"].append(out.copy())

    def __enter__(self):
        for name in self.NAMES:
            setattr(twodflag, name, getattr(self, name))
        return self

    def __exit__(self, *exc):
        for name, fn in self.orig.items():
            setattr(twodflag, name, fn)

    def arrays(self):
        """stage -> stacked (baseline, ...) array: float32, or packed flags."""
        out = {}
        for name, is_float in inputs.RECORDED_STAGES.items():
            stacked = np.stack(self.stages[name])
            out[name] = (stacked.astype(np.float32) if is_float
                         else np.packbits(stacked.astype(np.bool_)))  # fmt: skip
        return out


def _write(path, members):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(members):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(members[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())
    print("wrote", path, os.path.getsize(path), "bytes")


def check_oracle(n_draws: int) -> int:
    """Random small parameter sets through the reference and the oracle; returns the number
    of draws with a difference."""
    from oracle import twodflag_oracle as oracle

    bad = 0
    for draw in range(n_draws):
        rs = np.random.RandomState(1000 + draw)
        shape = (int(rs.randint(1, 25)), int(rs.randint(1, 70)), int(rs.randint(1, 3)))
        kind = str(rs.choice(["rfi", "nans", "quantised", "constant_zero",
                              "subnormal", "large", "nan_parts", "amplitudes", "negative"]))
        windows = [1, 2, 3, 4, 5, 8, 12, 16]
        params = {
            "outlier_nsigma": float(rs.choice([3.0, 4.5, 6.0])),
            "windows_time": [int(w) for w in rs.choice(windows, rs.randint(1, 6))],
            "windows_freq": [int(w) for w in rs.choice(windows, rs.randint(1, 6))],
            "background_reject": float(rs.choice([1.5, 2.0, 3.0])),
            "background_iterations": int(rs.randint(0, 4)),
            "spike_width_time": float(rs.choice([0.0, 2.0, 12.5, 40.0])),
            "spike_width_freq": float(rs.choice([0.0, 3.0, 10.0, 40.0])),
            "time_extend": int(rs.randint(0, 6)), "freq_extend": int(rs.randint(0, 7)),
            "freq_chunks": int(rs.choice([1, 2, 3, 10, 40])),
            "average_freq": int(rs.choice([1, 1, 2, 3, 7])),
            "flag_all_time_frac": float(rs.choice([0.0, 0.25, 0.6, 1.0])),
            "flag_all_freq_frac": float(rs.choice([0.0, 0.25, 0.8, 1.0])),
            "rho": float(rs.choice([1.0, 1.3, 2.0])),
        }  # fmt: skip
        data, flags = inputs.make_data(shape, kind, 2000 + draw)
        label = f"draw {draw}: {shape} {kind} {params}"
        try:
            ours, stages = oracle.flag(data, flags, **params)
        except ValueError as exc:  # every window clipped away
            print(label, "skipped:", exc)
            continue
        with _Spies() as spies:
            ref = reference_flagger(params).get_flags(data, flags)
        diff = [] if np.array_equal(ours, ref) else ["flags"]
        for name, is_float in inputs.RECORDED_STAGES.items():
            theirs = np.stack(spies.stages[name])
            if name == "unaveraged":
                mine = (stages["row_flags"] | stages["row_all"][:, :, None]
                        | stages["col_all"][:, None, :])  # fmt: skip
            else:
                mine = stages[name]
            if is_float:
                same = np.array_equal(theirs.astype(np.float32).view(np.uint32),
                                      mine.view(np.uint32))  # fmt: skip
            else:
                same = np.array_equal(theirs.astype(np.bool_), mine.astype(np.bool_))
            if not same:
                diff.append(name)
        bad += bool(diff)
        print(label, "MISMATCH " + " ".join(diff) if diff else "ok", flush=True)
    print(f"{n_draws} draws, {bad} with a mismatch")
    return bad


def main() -> None:
    if "--check-oracle" in sys.argv:
        sys.exit(1 if check_oracle(int(sys.argv[sys.argv.index("--check-oracle") + 1])) else 0)
    out = {"cases": np.array(json.dumps(inputs.case_list(), sort_keys=True))}
    stage_out = {}
    for case in inputs.case_list():
        name = case["name"]
        data, flags = inputs.make_case(name)
        stages = {"background": [], "time_flags": []}
        spies = _Spies() if name in inputs.STAGE_CASES else None
        if spies is not None:
            spies.__enter__()
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
            if spies is not None:
                spies.__exit__()
        if spies is not None:
            for stage, array in spies.arrays().items():
                stage_out[f"{name}_{stage}"] = array
        out[f"{name}_flags"] = np.packbits(result.astype(np.bool_))
        if name == inputs.STAGE_CASE:
            out[f"{name}_background"] = np.stack(stages["background"]).astype(np.float32)
            out[f"{name}_time_flags"] = np.packbits(np.stack(stages["time_flags"]))
        print(name, data.shape, int(result.sum()), "flags", flush=True)
    out["versions"] = np.array(f"numpy {np.__version__}")
    _write(inputs.GOLDEN, out)
    stage_out["cases"] = np.array(json.dumps(inputs.STAGE_CASES))
    _write(inputs.STAGES_GOLDEN, stage_out)


if __name__ == "__main__":
    main()
