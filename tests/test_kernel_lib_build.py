"""The helper headers for run-time compiled kernels (kernels/wg_reduce.h,
transpose_base.h, rank.h) and the package's own kernel templates (fill, hreduce), without a
GPU: every test kernel of tests/kernels/ and every template of accel.KERNEL_DIR is rendered
and compiled for gfx950 by hipcc, device side only, and the headers are checked to
include nothing that hiprtc would not find."""

import os
import re
import shutil
import subprocess

import pytest

from katsdpsigproc_amd import accel

KERNELS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kernels")
HEADERS = ["wg_reduce.h", "transpose_base.h", "rank.h"]

# One rendering per code path of the headers: the shuffle path inside a wavefront and
# across wavefronts, the LDS path for sizes that straddle wavefronts, every value type
# the reductions are exercised with, and the tile for each element size.
RENDERINGS = [
    ("reduce_test.hip.in", {"type": "int", "size": 64, "rows": 4, "op": "op_plus", "op2": "op_max",
                            "broadcast": "true", "shuffle": "true"}),
    ("reduce_test.hip.in", {"type": "int", "size": 87, "rows": 2, "op": "op_plus", "op2": "op_max",
                            "broadcast": "false", "shuffle": "true"}),
    ("reduce_test.hip.in", {"type": "float2", "size": 256, "rows": 1, "op": "op_plus", "op2": "op_plus",
                            "broadcast": "true", "shuffle": "true"}),
    ("reduce_test.hip.in", {"type": "long long", "size": 160, "rows": 1, "op": "op_plus", "op2": "op_min",
                            "broadcast": "true", "shuffle": "false"}),
    ("reduce_test.hip.in", {"type": "double", "size": 12, "rows": 21, "op": "op_fmin", "op2": "op_fmax",
                            "broadcast": "false", "shuffle": "false"}),
    ("reduce_test.hip.in", {"type": "unsigned", "size": 1, "rows": 256, "op": "op_fmin", "op2": "op_fmax",
                            "broadcast": "true", "shuffle": "true"}),
    ("rank_test.hip.in", {"size": 128, "store": 8, "shuffle": "true"}),
    ("rank_test.hip.in", {"size": 97, "store": 4, "shuffle": "false"}),
    ("transpose_test.hip.in", {"ctype": "unsigned char", "block": 8, "vtx": 2, "vty": 3}),
    ("transpose_test.hip.in", {"ctype": "float", "block": 16, "vtx": 4, "vty": 1}),
    ("transpose_test.hip.in", {"ctype": "double2", "block": 32, "vtx": 2, "vty": 2}),
]  # fmt: skip

# The package's own templates (accel.KERNEL_DIR) and the argument-passing test kernel. hreduce:
# every element type the operation is tested with, with an operator that suits it, at one row
# lane, at a partly filled last wavefront, at one wavefront per row and across wavefronts.
_HREDUCE_OPS = {
    "unsigned char": ("a | b", "0"), "short": ("min(a, b)", "32767"), "int": ("a + b", "0"),
    "long long": ("a + b", "0"), "unsigned long long": ("max(a, b)", "0"),
    "float": ("pick(a, b)", "INFINITY"), "double": ("a + b", "0.0"),
}  # fmt: skip
_PICK = "DEVICE_FN static inline float pick(float a, float b) { return fminf(a, b); }"
RENDERINGS += [
    ("hreduce.hip.in", {"type": ctype, "wgsx": wgsx, "wgsy": wgsy, "op": op, "identity": identity,
                        "extra_code": _PICK if ctype == "float" else ""})
    for wgsx, wgsy in [(1, 3), (16, 5), (64, 4), (512, 2)]
    for ctype, (op, identity) in _HREDUCE_OPS.items()
]  # fmt: skip
RENDERINGS += [
    ("fill.hip.in", {"ctype": ctype, "wgs": wgs})
    for ctype, wgs in [("unsigned char", 1024), ("short", 64), ("int", 96), ("long long", 64),
                       ("unsigned long long", 1), ("float", 256), ("double", 64), ("float2", 64),
                       ("double2", 128)]
]  # fmt: skip
RENDERINGS.append(("args_test.hip.in", {}))


def _rendering_id(name, keys):
    if name == "hreduce.hip.in":  # type and geometry tell these apart
        keys = {k: keys[k] for k in ("type", "wgsx", "wgsy")}
    return "-".join([name.split("_")[0].split(".")[0]] + [str(v).replace(" ", "") for v in keys.values()])


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc is not installed")
@pytest.mark.parametrize("name, keys", RENDERINGS,
                         ids=[_rendering_id(n, k) for n, k in RENDERINGS])
def test_kernels_compile_for_gfx950(name, keys, tmp_path):
    keys = dict(keys, simd_group_size=64)
    text = accel.render_template(name, keys, extra_dirs=[KERNELS])
    assert "$" not in text
    source = tmp_path / "kernel.hip"
    source.write_text(text)
    result = subprocess.run(
        ["hipcc", "--offload-arch=gfx950", "--cuda-device-only", "-O3", "-std=c++17",
         "-I" + accel.KERNEL_DIR, "-c", str(source), "-o", str(tmp_path / "kernel.o")],
        capture_output=True, text=True,
    )  # fmt: skip
    assert result.returncode == 0, result.stderr
    assert (tmp_path / "kernel.o").stat().st_size > 0


@pytest.mark.parametrize("header", HEADERS)
def test_headers_include_only_what_hiprtc_has(header):
    # hiprtc has no standard library: port.h, a sibling header and the HIP runtime only
    allowed = {'"port.h"', "<hip/hip_runtime.h>"} | {f'"{h}"' for h in HEADERS}
    with open(os.path.join(accel.KERNEL_DIR, header)) as f:
        includes = re.findall(r"^\s*#\s*include\s*(\S+)", f.read(), re.MULTILINE)
    assert includes and '"port.h"' in includes
    assert set(includes) <= allowed, set(includes) - allowed
