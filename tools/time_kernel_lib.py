#!/usr/bin/env python3
"""What kernels built from the helper headers (kernels/transpose_base.h, wg_reduce.h,
rank.h) cost next to the library's own operations, on inputs larger than the Infinity
Cache:

  transpose  a plain transposing copy from transpose_base.h, every (block, vtx, vty) of a
             small grid, against the native Transpose, at 16384 x 8192 float32
  rowsum     a row sum from wg_reduce.h (shuffle, no broadcast), a few work-group shapes,
             against HReduce at its autotuned shape, at 16384 x 4096 float32
  median     1.4826 * median_non_zero_float of |x| over 4096-channel rows from rank.h (256
             work-items, 16 values each in registers), against NoiseEstMADTDevice, at
             16384 baselines

Every configuration is timed with device events after a warm-up, the configurations
alternating within each round; the figure is the median over rounds. Each output is
checked against NumPy (transpose, row sum on integer-valued floats) or against the
native operation (median). The result is printed as Markdown tables.

usage: tools/time_kernel_lib.py [rounds]          time on the GPU
       tools/time_kernel_lib.py --resources       registers, scratch and LDS of the timed
                                                  kernels from the code-object metadata
                                                  (hipcc; needs no GPU)
       tools/time_kernel_lib.py --once            launch the two row sums once each (the
                                                  program for a rocprofv3 --pmc run; if
                                                  hiprtc does not find <hip/hip_runtime.h>
                                                  under the profiler, put the ROCm include
                                                  directory in CPATH)
       tools/time_kernel_lib.py --counters DIR    instructions per element from the
                                                  counter_collection.csv of that run
"""
import csv
import glob
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from katsdpsigproc_amd import accel  # noqa: E402

TRANSPOSE_SHAPE = (16384, 8192)
ROWS, COLUMNS = 16384, 4096
CALLS = 5

TRANSPOSE = """
#include "transpose_base.h"
KERNEL REQD_WORK_GROUP_SIZE(${block}, ${block}, 1) void lib_transpose(
    const GLOBAL float *RESTRICT in, GLOBAL float *RESTRICT out, int in_rows, int in_cols,
    int in_stride, int out_stride)
{
    LOCAL_DECL ksp::transpose_tile<float, ${block}, ${vtx}, ${vty}> tile;
    ksp::transpose_coords<${block}, ${vtx}, ${vty}> coords;
    coords.init_simple();
    coords.load([&](int r, int c, int lr, int lc) {
        if (r < in_rows && c < in_cols) tile.arr[lr][lc] = in[(long)r * in_stride + c];
    });
    BARRIER();
    coords.store([&](int r, int c, int lr, int lc) {
        if (r < in_cols && c < in_rows) out[(long)r * out_stride + c] = tile.arr[lr][lc];
    });
}
"""

ROWSUM = """
#include "wg_reduce.h"
KERNEL REQD_WORK_GROUP_SIZE(${wgsx}, ${wgsy}, 1) void lib_rowsum(
    const GLOBAL float *RESTRICT in, GLOBAL float *RESTRICT out, int n_cols, int in_stride)
{
    LOCAL_DECL ksp::wg_reduce_scratch<float, ${wgsx}, true> scratch[${wgsy}];
    const int row = get_global_id(1), idx = get_local_id(0);
    const GLOBAL float *src = in + (long)in_stride * row;
    float value = 0.0f;
    for (int c = idx; c < n_cols; c += ${wgsx}) value += src[c];
    value = ksp::wg_reduce<float, ${wgsx}, ksp::op_plus, false, true>(
        value, idx, &scratch[get_local_id(1)]);
    if (idx == 0) out[row] = value;
}
"""

MEDIAN = """
#include "rank.h"
#define WGS 256
#define PER (${channels} / WGS)
KERNEL REQD_WORK_GROUP_SIZE(WGS, 1, 1) void lib_madnz(
    const GLOBAL float *RESTRICT in, GLOBAL float *RESTRICT out, int in_stride)
{
    typedef ksp::ranker_serial_store<float, PER> serial_t;
    typedef ksp::ranker_parallel<serial_t, float, WGS, true> ranker_t;
    LOCAL_DECL ranker_t::scratch_type scratch;
    const int idx = get_local_id(0);
    const GLOBAL float *src = in + (long)in_stride * get_group_id(0);
    serial_t serial;
#pragma unroll
    for (int i = 0; i < PER; i++) serial[i] = __builtin_fabsf(src[i * WGS + idx]);
    const ranker_t ranker(serial, &scratch, idx);
    const float m = ksp::median_non_zero_float<true>(ranker, ${channels});
    // scaled in float64 and rounded once, as the native kernel does
    if (idx == 0) out[get_group_id(0)] = (float)(1.4826 * (double)m);
}
"""

TILINGS = [(b, x, y) for b in (16, 32) for x in (1, 2, 4) for y in (1, 2, 4)]
ROWSUM_SHAPES = [(32, 8), (64, 4), (64, 8), (64, 16), (128, 2), (128, 4), (128, 8), (256, 1), (256, 4)]
# what --resources and --once use unless told otherwise: the shapes that timed best
BEST_TILING = (16, 2, 1)
BEST_ROWSUM = (128, 2)


def _keys(kind, geometry):
    if kind == "transpose":
        return dict(zip(("block", "vtx", "vty"), geometry))
    if kind == "rowsum":
        return dict(zip(("wgsx", "wgsy"), geometry))
    return {"channels": COLUMNS}


SOURCES = {"transpose": TRANSPOSE, "rowsum": ROWSUM, "median": MEDIAN}


class Timed:
    """A callable launch, its name, the bytes it moves and a check of its output."""

    def __init__(self, group, name, run, check, n_bytes):
        self.group, self.name, self.run, self.check, self.n_bytes = group, name, run, check, n_bytes
        self.times = []


def _device(ctx, q, ary):
    out = accel.DeviceArray(ctx, ary.shape, ary.dtype)
    out.set(q, ary)
    return out


def _setup_transpose(ctx, q, rng, tilings):
    from katsdpsigproc_amd import transpose

    timed = []
    rows, cols = TRANSPOSE_SHAPE
    host = rng.integers(0, 1 << 20, (rows, cols)).astype(np.float32)
    native = transpose.TransposeTemplate(ctx, np.float32, "float").instantiate(q, (rows, cols))
    native.ensure_all_bound()
    native.buffer("src").set(q, host)
    src, dest = native.buffer("src"), native.buffer("dest")
    n_bytes = 2 * host.nbytes

    def check_transpose():
        out = dest.get(q)
        ok = np.array_equal(out[:64], host[:, :64].T) and np.array_equal(out[-64:], host[:, -64:].T)
        dest.zero(q)
        return "matches" if ok else "MISMATCH"

    timed.append(Timed("transpose", "native Transpose (64 x 64 tile)", native, check_transpose, n_bytes))
    for block, vtx, vty in tilings:
        kernel = accel.build(ctx, "lib_transpose", _keys("transpose", (block, vtx, vty)),
                             source=TRANSPOSE).get_kernel("lib_transpose")  # fmt: skip
        args = [src.buffer, dest.buffer, np.int32(rows), np.int32(cols),
                np.int32(src.padded_shape[1]), np.int32(dest.padded_shape[1])]  # fmt: skip
        gsize = (accel.divup(cols, block * vtx) * block, accel.divup(rows, block * vty) * block)

        def run(kernel=kernel, args=args, gsize=gsize, block=block):
            q.enqueue_kernel(kernel, args, global_size=gsize, local_size=(block, block))

        timed.append(Timed("transpose", f"transpose_base.h {block} x {block}, vtx {vtx}, vty {vty}",
                           run, check_transpose, n_bytes))  # fmt: skip
    return timed


def _setup_rowsum(ctx, q, rng, rowsum_shapes):
    from katsdpsigproc_amd import reduce

    timed = []
    # integer-valued floats, so that any order of summation is exact
    host = rng.integers(0, 256, (ROWS, COLUMNS)).astype(np.float32)
    sums = host.sum(axis=1, dtype=np.float64).astype(np.float32)
    hreduce = reduce.HReduceTemplate(ctx, np.float32, "float", "a + b", "0.0f")
    native = hreduce.instantiate(q, (ROWS, COLUMNS))
    native.ensure_all_bound()
    native.buffer("src").set(q, host)
    rsrc, rdest = native.buffer("src"), native.buffer("dest")

    def check_rowsum():
        ok = np.array_equal(rdest.get(q), sums)
        rdest.zero(q)
        return "matches" if ok else "MISMATCH"

    timed.append(Timed("rowsum", f"HReduce, autotuned {hreduce.wgsx} x {hreduce.wgsy}", native,
                       check_rowsum, host.nbytes))  # fmt: skip
    for wgsx, wgsy in rowsum_shapes:
        kernel = accel.build(ctx, "lib_rowsum", _keys("rowsum", (wgsx, wgsy)),
                             source=ROWSUM).get_kernel("lib_rowsum")  # fmt: skip
        args = [rsrc.buffer, rdest.buffer, np.int32(COLUMNS), np.int32(rsrc.padded_shape[1])]

        def run(kernel=kernel, args=args, wgsx=wgsx, wgsy=wgsy):
            q.enqueue_kernel(kernel, args, global_size=(wgsx, ROWS), local_size=(wgsx, wgsy))

        timed.append(Timed("rowsum", f"wg_reduce.h {wgsx} x {wgsy}", run, check_rowsum, host.nbytes))
    return timed


def _setup_median(ctx, q, rng):
    from katsdpsigproc_amd.rfi import device

    timed = []
    host = rng.standard_normal((ROWS, COLUMNS), dtype=np.float32)
    host[rng.random((ROWS, COLUMNS), dtype=np.float32) < 0.1] = 0.0
    native = device.NoiseEstMADTDeviceTemplate(ctx, COLUMNS).instantiate(q, COLUMNS, ROWS)
    native.ensure_all_bound()
    native.buffer("deviations").set(q, host)
    msrc, mdest = native.buffer("deviations"), native.buffer("noise")
    native()
    noise = np.array(mdest.get(q))
    lo = np.abs(host[:16])
    expected = np.array([np.median(r[r > 0]) for r in lo], np.float32) * np.float32(1.4826)
    assert np.allclose(noise[:16], expected, rtol=1e-6), "NoiseEstMADTDevice disagrees with NumPy"

    def check_median():
        out = np.array(mdest.get(q))
        mdest.zero(q)
        if np.array_equal(out, noise):
            return "matches"
        same = float(np.mean(out == noise))
        close = np.allclose(out, noise, rtol=3e-7, atol=0)
        return f"{'within 3e-7' if close else 'MISMATCH'} ({100 * same:.2f} % identical)"

    timed.append(Timed("median", "NoiseEstMADTDevice", native, check_median, host.nbytes))
    kernel = accel.build(ctx, "lib_madnz", _keys("median", None), source=MEDIAN).get_kernel("lib_madnz")
    args = [msrc.buffer, mdest.buffer, np.int32(msrc.padded_shape[1])]

    def run_median():
        q.enqueue_kernel(kernel, args, global_size=(256 * ROWS,), local_size=(256,))

    timed.append(Timed("median", "rank.h median_non_zero_float, 256 work-items", run_median,
                       check_median, host.nbytes))  # fmt: skip
    return timed


def time_all(rounds):
    ctx = accel.create_some_context(False)
    q = ctx.create_command_queue()
    rng = np.random.default_rng(61)
    timed = (_setup_transpose(ctx, q, rng, TILINGS) + _setup_rowsum(ctx, q, rng, ROWSUM_SHAPES)
             + _setup_median(ctx, q, rng))  # fmt: skip
    ok = {}
    for t in timed:  # warm-up, and each output checked on its own, the destination cleared after
        t.run()
        t.run()
        ok[t.name] = t.check()
    q.finish()
    for _ in range(rounds):
        for t in timed:
            a = q.enqueue_marker()
            for _ in range(CALLS):
                t.run()
            e = q.enqueue_marker()
            q.finish()
            t.times.append(1e3 * e.time_since(a) / CALLS)

    print(f"Measured on {ctx.device.name}: {rounds} rounds x {CALLS} calls per configuration, "
          "alternating; median (minimum) per call.\n")  # fmt: skip
    shapes = {"transpose": "%d x %d float32" % TRANSPOSE_SHAPE,
              "rowsum": f"{ROWS} x {COLUMNS} float32",
              "median": f"{ROWS} rows of {COLUMNS} float32"}  # fmt: skip
    for group in ("transpose", "rowsum", "median"):
        members = [t for t in timed if t.group == group]
        base = float(np.median(members[0].times))
        print(f"### {group}: {shapes[group]}\n")
        print("| kernel | ms | min ms | GB/s | time / yardstick | output |")
        print("|---|---|---|---|---|---|")
        for t in members:
            ms = float(np.median(t.times))
            print(f"| {t.name} | {ms:.4f} | {min(t.times):.4f} | {t.n_bytes / (ms * 1e6):.0f} | "
                  f"{ms / base:.2f} | {ok[t.name]} |")
        print()
    if any(v.startswith("MISMATCH") for v in ok.values()):
        sys.exit(1)


def once():
    ctx = accel.create_some_context(False)
    q = ctx.create_command_queue()
    for t in _setup_rowsum(ctx, q, np.random.default_rng(61), [BEST_ROWSUM]):
        t.run()
        q.finish()
        print(t.name, t.check())


def counters(directory):
    files = glob.glob(os.path.join(directory, "**", "*counter_collection.csv"), recursive=True)
    if not files:
        sys.exit(f"no counter_collection.csv under {directory}")
    totals = {}
    for name in files:
        with open(name) as f:
            for row in csv.DictReader(f):
                kernel = row["Kernel_Name"].split("(")[0]
                if kernel not in ("hreduce", "lib_rowsum"):
                    continue
                # the launch of --once is the kernel's last dispatch (an autotuning pass of
                # HReduce, if its result was not cached, comes before it)
                per_kernel = totals.setdefault(kernel, {})
                dispatch = int(row["Dispatch_Id"])
                if dispatch >= per_kernel.get(row["Counter_Name"], (-1, 0.0))[0]:
                    per_kernel[row["Counter_Name"]] = (dispatch, float(row["Counter_Value"]))
    elements = ROWS * COLUMNS
    print(f"Wavefront instructions per element ({ROWS} x {COLUMNS} elements, one launch):\n")
    names = sorted({c for v in totals.values() for c in v})
    print("| kernel | " + " | ".join(names) + " | sum |")
    print("|---|" + "---|" * (len(names) + 1))
    for kernel, values in sorted(totals.items()):
        means = [values.get(c, (0, 0.0))[1] / elements for c in names]
        insts = sum(m for m, c in zip(means, names) if c.startswith("SQ_INSTS"))
        print(f"| {kernel} | " + " | ".join(f"{m:.5f}" for m in means) + f" | {insts:.5f} |")


def resources():
    """Compile the three timed kernels as accel.build does (-O3 -std=c++17, for gfx950) and
    read registers, scratch and LDS from the AMDGPU metadata note of the code object."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    readelf = os.path.join(rocm, "llvm", "bin", "llvm-readelf")
    print("| kernel | VGPRs | AGPRs | SGPRs | scratch bytes | LDS bytes |")
    print("|---|---|---|---|---|---|")
    for kind, geometry in (("transpose", BEST_TILING), ("rowsum", BEST_ROWSUM), ("median", None)):
        text = accel.render_template(kind, _keys(kind, geometry), source=SOURCES[kind])
        with tempfile.TemporaryDirectory() as tmp:
            src, obj = os.path.join(tmp, "k.hip"), os.path.join(tmp, "k.co")
            with open(src, "w") as f:
                f.write(text)
            subprocess.run(["hipcc", "--offload-arch=gfx950", "--cuda-device-only",
                            "--no-gpu-bundle-output", "-O3", "-std=c++17", "-I" + accel.KERNEL_DIR,
                            "-c", src, "-o", obj], check=True)  # fmt: skip
            notes = subprocess.run([readelf, "--notes", obj], check=True, capture_output=True,
                                   text=True).stdout  # fmt: skip

        def field(name):
            return int(re.search(r"\.%s:\s*(\d+)" % name, notes).group(1))

        label = kind if geometry is None else f"{kind} {' x '.join(map(str, geometry))}"
        print(f"| {label} | {field('vgpr_count')} | {field('agpr_count')} | {field('sgpr_count')} | "
              f"{field('private_segment_fixed_size')} | {field('group_segment_fixed_size')} |")


if __name__ == "__main__":
    if "--resources" in sys.argv:
        resources()
    elif "--once" in sys.argv:
        once()
    elif "--counters" in sys.argv:
        counters(sys.argv[sys.argv.index("--counters") + 1])
    else:
        time_all(int(sys.argv[1]) if len(sys.argv) > 1 else 7)
