#!/usr/bin/env python3
"""Generate ``rfi_masked_filter_golden.npz``: results of the REAL reference
``katsdpsigproc.rfi.twodflag.masked_gaussian_filter`` for the cases of
``tests/inputs_masked_filter.py``.

The reference is numba code. It runs as plain Python when a stub ``numba`` module is
imported first, the recipe of ``make_golden_twodflag.py``. Run in the build container only
(the reference never travels to the GPU box):

    PYTHONPATH=<reference>/src python3 tests/golden/make_golden_masked_filter.py

One adjustment makes plain NumPy compute what the numba-compiled reference computes:
``_box_gaussian_filter1d`` gets its ``passes`` as an object whose ``T(d) ** passes`` is
numba's ``int_power_impl``, squaring and multiplying in the data's type ``T`` (NumPy's
float32 power rounds 69 ** 4 to 22667122, numba's gives 22667120).

The archive holds the outputs only (the inputs are seeded), with fixed member timestamps,
so that a rerun reproduces it byte for byte.
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

from tests import inputs_masked_filter as inputs  # noqa: E402


class _NumbaPasses:
    """The number of passes, as an integer for everything the reference does with it
    except that a NumPy scalar raised to it is numba's power: repeated squaring in the
    scalar's type."""

    __array_ufunc__ = None  # NumPy scalars defer to __rpow__ and __rmul__
    powers = 0

    def __init__(self, value):
        self.value = int(value)

    def __index__(self):
        return self.value

    def __eq__(self, other):
        return self.value == other

    def __hash__(self):
        return hash(self.value)

    def __add__(self, other):
        return self.value + other

    def __rmul__(self, other):
        return other * self.value

    def __mul__(self, other):
        return self.value * other

    def __rpow__(self, base):
        scalar = type(base)
        assert scalar in (np.float32, np.float64), scalar
        result, e = scalar(1), self.value
        while e:
            if e & 1:
                result = scalar(result * base)
            base = scalar(base * base)
            e >>= 1
        _NumbaPasses.powers += 1
        return result


def _with_numba_power(box1d):
    def wrapper(data, r, out, passes):
        return box1d(data, r, out, _NumbaPasses(passes))

    return wrapper


twodflag._box_gaussian_filter1d = _with_numba_power(twodflag._box_gaussian_filter1d)


def _write(path, members):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(members):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(members[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(info, buf.getvalue())
    print("wrote", path, os.path.getsize(path), "bytes")


def reference(data, flags, sigma, passes):
    out = np.empty_like(data)
    before = _NumbaPasses.powers
    with np.errstate(all="ignore"):
        twodflag.masked_gaussian_filter(data.copy(), flags.copy(), np.array(sigma, np.float64),
                                        out, passes=passes)
    filtered = sum(inputs.radius(s, passes) > 0 for s in sigma)
    assert filtered == 0 or _NumbaPasses.powers > before, "the power did not go through numba's"
    return out


def main() -> None:
    out = {"cases": np.array(json.dumps(inputs.case_list(), sort_keys=True))}
    for case in inputs.case_list():
        name = case["name"]
        data, flags = inputs.make_case(name)
        result = reference(data, flags, case["sigma"], case["passes"])
        assert result.dtype == data.dtype
        out[name] = result
        print(name, data.shape, data.dtype, "passes", case["passes"],
              int(np.isnan(result).sum()), "NaN", flush=True)  # fmt: skip
    out["versions"] = np.array(f"numpy {np.__version__}")
    _write(inputs.GOLDEN, out)


if __name__ == "__main__":
    main()
