"""The helper headers for run-time compiled kernels (kernels/wg_reduce.h,
transpose_base.h, rank.h), without a GPU: every test kernel of tests/kernels/ is rendered
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


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc is not installed")
@pytest.mark.parametrize("name, keys", RENDERINGS,
                         ids=["-".join([n.split("_")[0]] + [str(v).replace(" ", "") for v in k.values()])
                              for n, k in RENDERINGS])  # fmt: skip
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
