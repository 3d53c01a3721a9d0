#!/usr/bin/env python3
"""Time the 2-D SumThreshold flagger's device operation (default parameters).

Prints ms per call and input samples/s for a calibration-like block of
100 x 4096 x 2016 complex64 and for 32 x 32768 x 64, and the VGPR / scratch use of each
``tdf_*`` kernel from the code-object metadata. Usage:
``python tools/time_twodflag.py [--reps N] [--json OUT]``.
"""

import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from katsdpsigproc_amd import accel  # noqa: E402
from katsdpsigproc_amd.rfi import twodflag  # noqa: E402

SHAPES = [(100, 4096, 2016), (32, 32768, 64)]


def kernel_resources():
    """VGPRs and scratch bytes per lane of every tdf_ kernel (hipcc resource remarks)."""
    src = os.path.join(ROOT, "katsdpsigproc_amd", "csrc", "twodflag.hip")
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
           "-fhip-fp32-correctly-rounded-divide-sqrt", "--cuda-device-only", "-c", src,
           "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]  # fmt: skip
    try:
        text = subprocess.run(cmd, capture_output=True, text=True, check=False).stderr
    except OSError as exc:
        return {"error": str(exc)}
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = re.sub(r"^_ZN12_GLOBAL__N_1\d+", "", m.group(1))
            out[name] = {}
        m = re.search(r"(VGPRs|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name:
            out[name]["vgpr" if m.group(1) == "VGPRs" else "scratch"] = int(m.group(2))
    return out


def time_shape(context, queue, shape, reps):
    rs = np.random.RandomState(1)
    n_time, n_freq, n_bl = shape
    op = twodflag.SumThresholdFlaggerDeviceTemplate(context).instantiate(queue, *shape)
    op.ensure_all_bound()
    data = np.empty(shape, np.complex64)
    for t in range(n_time):
        data[t] = (2.0 + rs.standard_normal((n_freq, n_bl)) * 0.1).astype(np.float32)
    op.buffer("data").set(queue, data)
    op.buffer("input_flags").set(queue, np.zeros(shape, np.uint8))
    del data
    op()
    queue.finish()
    t0 = time.perf_counter()
    for _ in range(reps):
        op()
    queue.finish()
    ms = (time.perf_counter() - t0) / reps * 1e3
    samples = n_time * n_freq * n_bl
    return {"shape": list(shape), "batch": op.batch, "workspace_bytes": op.workspace_bytes,
            "ms_per_call": ms, "samples_per_s": samples / (ms * 1e-3),
            "flag_fraction": float(op.buffer("flags").get(queue).mean())}  # fmt: skip


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--reps", type=int, default=3)
    parser.add_argument("--json")
    args = parser.parse_args()
    context = accel.create_some_context(interactive=False)
    queue = context.create_command_queue()
    result = {"device": context.device.name, "runs": [], "kernels": kernel_resources()}
    for shape in SHAPES:
        r = time_shape(context, queue, shape, args.reps)
        result["runs"].append(r)
        print(f"{r['shape']}: {r['ms_per_call']:.1f} ms/call, {r['samples_per_s']:.3g} samples/s "
              f"(batch {r['batch']})", flush=True)  # fmt: skip
    for name, res in sorted(result["kernels"].items()):
        print(f"{name}: {res}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
